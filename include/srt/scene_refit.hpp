// srt/scene_refit.hpp -- C++ mirror of include/srt_scene_refit.h: AssetUtils::SceneRefit, used as
// AssetUtils::UploadModelDataToGPU is -- it uploads the models to the Compute in use -- and then refits that
// upload to device vertices, frame after frame, instead of AssetUtils::RefitBVH and a second upload.  Errors throw
// std::runtime_error carrying srt_last_error().
//
//   c.Use();
//   AssetUtils::SceneRefit scene({model.get()}, 5);      // = UploadModelDataToGPU({model.get()}, 5)
//   ... per frame: scene.Refit(verts_dev, n_verts); c.Dispatch(W / 8, H / 8); ...
#pragma once

#include <utility>
#include <vector>

#include "../srt_scene_refit.h"
#include "srt.hpp"

namespace srt {
namespace AssetUtils {

class SceneRefit {
 public:
  explicit SceneRefit(const std::vector<Model*>& models, const uint32_t binding_offset = 0) {
    (void)binding_offset;  // bindings are fixed by the C ABI
    Graphics::Compute* c = Graphics::detail::current();
    if (!c) throw std::runtime_error("SceneRefit: no Compute in use");
    std::vector<const srt_model*> hs;
    for (Model* m : models) {
      if (!m) throw std::runtime_error("Model was null!");
      hs.push_back(m->handle());
    }
    srt_scene* s = nullptr;
    check(srt_scene_build(hs.data(), (uint32_t)hs.size(), &s), "SceneRefit");
    const int rc = srt_upload_scene_obj_refit(c->context(), s, &r_);
    srt_scene_free(s);
    check(rc, "SceneRefit");
  }
  SceneRefit(const SceneRefit&) = delete;
  SceneRefit& operator=(const SceneRefit&) = delete;
  SceneRefit(SceneRefit&& o) noexcept : r_(std::exchange(o.r_, nullptr)) {}
  ~SceneRefit() {
    if (r_) srt_scene_refit_destroy(r_);
  }

  // srt_scene_refit: `verts_dev` is a device array of n_verts srt_vertex records, ready on the Compute's stream.
  void Refit(const srt_vertex* verts_dev, uint32_t n_verts, bool read_roots = false) {
    check(srt_scene_refit(r_, verts_dev, n_verts, read_roots ? SRT_SCENE_REFIT_READ_ROOTS : 0u), "SceneRefit::Refit");
  }
  int GetInt(const char* name) const {
    int v = 0;
    check(srt_scene_refit_get_int(r_, name, &v), "SceneRefit::GetInt");
    return v;
  }
  struct srt_scene_refit* handle() const { return r_; }

 private:
  struct srt_scene_refit* r_ = nullptr;
};

}  // namespace AssetUtils
}  // namespace srt
