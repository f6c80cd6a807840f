// capi_objects.hpp -- the opaque producer handles of include/srt_amd.h, for the units that take one apart: capi.cpp,
// which makes them, and scene_refit.hip (srt_upload_scene_obj_refit).
#pragma once

#include <memory>

#include "srt_internal.hpp"

struct srt_model {
  std::unique_ptr<srt::Model> m;
};
struct srt_scene {
  std::unique_ptr<srt::Scene> s;
};
