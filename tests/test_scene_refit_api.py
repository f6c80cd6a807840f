"""The scene refit's boundary (include/srt_scene_refit.h), CPU only: exported symbols and the version, the argument
errors reachable without a device, the unchanged code hash, the scene image's bytes after BuildSceneImage's body
moved behind scene_image_maps.hpp, the host schedule builder under ASan/UBSan as a stand-alone program, the build
defaults scene_refit.hip restates against their originals, and the header and its C++ mirror through a compiler."""
import ctypes as C
import re
import subprocess

from conftest import OBJECTS, PKG, ROOT
from srt_amd import _lib

NAMES = ["srt_scene_refit_abi_version", "srt_upload_scene_refit", "srt_upload_scene_obj_refit", "srt_scene_refit_destroy",
         "srt_scene_refit", "srt_scene_refit_get_int", "srt_scene_copy_device", "srt_scene_device_bytes"]


def declared_functions():
    text = (ROOT / "include" / "srt_scene_refit.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(srt_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_and_binding():
    assert declared_functions() == sorted(NAMES) == sorted(_lib.SCENE_REFIT_SYMBOLS)
    for other in (_lib.EXPORTED_SYMBOLS, _lib.QUERY_SYMBOLS, _lib.REFIT_SYMBOLS, _lib.SURFACE_REFIT_SYMBOLS):
        assert not set(NAMES) & set(other)
    out = subprocess.run(["nm", "-D", "--defined-only", str(PKG / "libsrt_amd.so")], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [n for n in NAMES if n not in exported]
    lib = _lib.lib()
    assert lib.srt_scene_refit_abi_version() == 1
    # the additive header leaves the other versions alone
    assert lib.srt_abi_version() == 2 and lib.srt_query_abi_version() == 1 and lib.srt_refit_abi_version() == 1
    header = (ROOT / "include" / "srt_scene_refit.h").read_text()
    assert "#define SRT_SCENE_REFIT_ABI_VERSION 1" in header and "#define SRT_SCENE_REFIT_READ_ROOTS 1u" in header
    assert _lib.SRT_SCENE_REFIT_READ_ROOTS == 1


def test_null_arguments_without_a_device():
    lib = _lib.lib()
    inv = _lib.SRT_ERR_INVALID
    v, h = C.c_int(7), C.c_void_p(0x1234)
    sizes = (C.c_size_t * 3)(1, 2, 3)
    buf = (C.c_uint8 * 64)()
    assert lib.srt_scene_refit(None, buf, 2, 0) == inv
    assert lib.srt_scene_refit(None, None, 0, _lib.SRT_SCENE_REFIT_READ_ROOTS) == inv
    assert lib.srt_scene_refit_destroy(None) == inv
    assert lib.srt_scene_refit_get_int(None, b"refit.count", C.byref(v)) == inv and v.value == 7
    assert lib.srt_scene_copy_device(None, buf, None, None) == inv
    assert lib.srt_scene_device_bytes(None, sizes) == inv and list(sizes) == [1, 2, 3]
    # no context: nothing is uploaded, and the handle comes back NULL
    assert lib.srt_upload_scene_refit(None, None, 0, None, 0, None, None, 0, None, 0, None, 0, C.byref(h)) == inv
    assert h.value is None
    h = C.c_void_p(0x1234)
    assert lib.srt_upload_scene_obj_refit(None, None, C.byref(h)) == inv and h.value is None


def test_python_mirror_needs_a_bound_object():
    import pytest

    import srt_amd as S
    c = S.Compute()  # never initialised: no context, no device
    with pytest.raises(RuntimeError):
        c.refit(None)
    with pytest.raises(RuntimeError):
        c.refit_get_int("refit.count")
    assert "refit" in S.Compute.bind_scene.__code__.co_varnames
    assert S.Compute.bind_scene.__defaults__ == (False,)  # the default is the plain upload


def test_code_hash_is_unchanged():
    """`make -s hash` -- the preprocessed pathtrace.hip translation unit and the hipcc flags -- still equals every
    code_hash stamped into profiles/counters.json: the refit lives in translation units and headers of its own."""
    h = subprocess.run(["make", "-s", "-C", str(PKG), "hash"], capture_output=True, text=True, check=True).stdout.strip()
    assert re.fullmatch(r"[0-9a-f]{16}", h)
    stamped = set(re.findall(r'"code_hash"\s*:\s*"([0-9a-f]+)"', (ROOT / "profiles" / "counters.json").read_text()))
    assert stamped == {h}, (stamped, h)
    # and none of pathtrace.hip's headers reads the new ones
    for name in ("pathtrace.hip", "context.hpp", "scene_image.hpp", "scene_layout.hpp", "launch_plan.hpp",
                 "srt_internal.hpp", "kernels.hpp", "traversal.hpp"):
        text = (PKG / "csrc" / name).read_text()
        assert "scene_refit" not in text and "scene_image_maps" not in text and "refit_fold" not in text, name


def test_scene_image_bytes_are_the_pinned_ones():
    """BuildSceneImage is now a call to BuildSceneImageMaps: tests/cpp/test_scene_image.cpp, untouched, still finds
    the 60 fingerprints of the arrays the upload sent before that code was host-only."""
    from test_producers import _sanitized_host_program

    text = (PKG / "csrc" / "scene_image.cpp").read_text()
    assert re.search(r"void BuildSceneImage\([^{]*\{\s*BuildSceneImageMaps\([^;]*nullptr\);\s*\}", text)
    exe = _sanitized_host_program("test_scene_image", ["scene_image.cpp", "scene_layout.cpp", "scene.cpp"],
                                  ["-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"])
    r = subprocess.run([str(exe), str(OBJECTS / "Rubik" / "Rubik.obj")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "scene image checks OK (60 images pinned)" in r.stdout


def test_schedule_builder_under_sanitizers():
    """tests/cpp/test_scene_refit_host.cpp with csrc/scene_refit_host.cpp linked directly, AddressSanitizer + UBSan,
    as a stand-alone program (`make SAN=1 test_scene_refit_host`: host code only, nothing preloaded)."""
    r = subprocess.run(["make", "-s", "-C", str(PKG), "SAN=1", "-j8", "test_scene_refit_host"], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "test_scene_refit_host: OK" in r.stdout


def test_restated_build_defaults_equal_the_originals():
    """scene_refit.hip cannot include kernels.hpp (it defines kernels), so it restates three macro defaults and the
    ring rule that pathtrace.hip and kernels.hpp hold.  BuildSceneImage sizes the top region from them: the copies
    must be the originals, token for token."""
    def default_of(text, macro):
        m = re.search(r"#ifndef %s\s*\n#define %s (\S+)\s*\n#endif" % (macro, macro), text)
        assert m, macro
        return m.group(1)

    mine = (PKG / "csrc" / "scene_refit.hip").read_text()
    pathtrace = (PKG / "csrc" / "pathtrace.hip").read_text()
    kernels = (PKG / "csrc" / "kernels.hpp").read_text()
    assert default_of(mine, "SRT_LDS_BLOCK") == default_of(pathtrace, "SRT_LDS_BLOCK")
    assert default_of(mine, "SRT_GW5_BLOCK") == default_of(pathtrace, "SRT_GW5_BLOCK")
    assert default_of(mine, "SRT_RING_GW5") == default_of(kernels, "SRT_RING_GW5")
    rule = r"\(int gw\) \{ return \(gw > 4 \|\| SRT_COOP\) \? SRT_RING_GW5 : (?:srt::)?kShortStack; \}"
    assert re.search(r"global_ring" + rule, kernels) and re.search(r"RingOf" + rule, mine)
    # the two units fill the struct from the same names, in the same order (pool_trav_lanes and the block sizes
    # size a launch; the image reads neither pool_trav_lanes nor lds_block)
    want = re.search(r"kBuild = \{kLdsBlock, kGw5Block, srt::kNodeBlkF4, srt::global_ring\(4\), srt::global_ring\(5\),\s*"
                     r"SRT_COOP != 0, srt::kCoopWaveBytes, srt::kCoopIdxBits, srt::kPoolTravLanes,\s*"
                     r"srt::kNodePad, \(uint32_t\)srt::kTriPad, srt::kTreeletCnt\};", pathtrace)
    got = re.search(r"kBuild = \{SRT_LDS_BLOCK, SRT_GW5_BLOCK, srt::kNodeBlkF4, RingOf\(4\), RingOf\(5\),\s*"
                    r"SRT_COOP != 0, srt::kCoopWaveBytes, srt::kCoopIdxBits, 0,\s*"
                    r"srt::kNodePad, \(uint32_t\)srt::kTriPad, srt::kTreeletCnt\};", mine)
    assert want and got
    image = (PKG / "csrc" / "scene_image.cpp").read_text() + (PKG / "csrc" / "scene_image.hpp").read_text()
    assert "pool_trav_lanes" not in image and "lds_block" not in image


def test_headers_compile_as_c_and_the_mirror_as_cxx(tmp_path):
    """include/srt_scene_refit.h under a C compiler (the struct tag beside the function of its name) and the C++
    mirror include/srt/scene_refit.hpp, syntax only."""
    c = tmp_path / "hdr.c"
    c.write_text('#include "srt_scene_refit.h"\n'
                 "int f(struct srt_scene_refit* r) { return srt_scene_refit(r, 0, 0, SRT_SCENE_REFIT_READ_ROOTS); }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", str(ROOT / "include"), str(c)], check=True)
    cxx = tmp_path / "mirror.cpp"
    cxx.write_text('#include "srt/scene_refit.hpp"\n'
                   "void f(srt::AssetUtils::Model* m, const srt_vertex* v) {\n"
                   "  srt::AssetUtils::SceneRefit s({m}, 5);\n"
                   '  s.Refit(v, 3);\n  s.Refit(v, 3, true);\n  (void)s.GetInt("refit.count");\n'
                   "  srt::AssetUtils::SceneRefit t(std::move(s));\n  (void)t.handle();\n}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", str(ROOT / "include"), str(cxx)],
                   check=True)
