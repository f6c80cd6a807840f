"""The sorted ray queries' boundary (include/srt_query_sort.h), CPU only: exported symbols, the host mirror srt_ray_order
against a numpy restatement of its rule (tests/ray_order_ref.py) -- order, keys and bounds, dword for dword -- the host
mirror under ASan/UBSan as a stand-alone program, the C header as C, the C++ mirror, and argument errors without a device."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import ray_order_ref as RO
import special_rays as SR
import srt_amd as S
from conftest import OBJECTS, PKG, ROOT
from srt_amd import _lib

NAMES = ["srt_query_sort_abi_version", "srt_query_closest_sorted", "srt_query_occluded_sorted", "srt_ray_order",
         "srt_query_copy_ray_order"]
F = np.float32


def rule_bits():
    """The two bit counts the rule names once (csrc/ray_order_rule.hpp); a device object reports them through get_int."""
    text = (PKG / "csrc" / "ray_order_rule.hpp").read_text()
    ob = int(re.search(r"#define SRT_RAY_ORIGIN_BITS (\d+)", text).group(1))
    db = int(re.search(r"#define SRT_RAY_DIR_BITS (\d+)", text).group(1))
    return ob, db


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_against_restatement(rays):
    """srt_ray_order == the restatement in order, keys and bounds; a permutation; equal keys keep the input order."""
    ob, db = rule_bits()
    order, keys, box = S.ray_order(rays, bounds=True)
    r_order, r_keys, r_box = RO.ray_order(rays, ob, db)
    assert (bits(box) == bits(r_box)).all(), (box, r_box)
    assert (keys == r_keys).all(), f"{(keys != r_keys).sum()} keys differ"
    assert (order == r_order).all()
    n = len(rays)
    assert sorted(order.tolist()) == list(range(n))
    assert (np.diff(keys.astype(np.int64)) >= 0).all()
    same = np.diff(keys.astype(np.int64)) == 0
    assert (np.diff(order.astype(np.int64))[same] > 0).all()
    assert (keys < (1 << 3 * (ob + db))).all()
    return order, keys, box


@pytest.fixture(scope="module")
def rubik_scene():
    return S.Scene.from_models([S.load_obj(OBJECTS / "Rubik" / "Rubik.obj")])


@pytest.fixture(scope="module")
def surface_rays(rubik_scene):
    """Rays that hit Rubik followed by rays from a sphere around it: origins spread over space."""
    lo, hi = SR.root_box(rubik_scene)
    hit, _, _ = SR.hitting_rays(rubik_scene, 2048, 11)
    return np.concatenate([hit, SR.sphere_rays(lo, hi, 4099 - len(hit), 12)])


def test_library_exports_and_binding():
    text = (ROOT / "include" / "srt_query_sort.h").read_text()
    assert "#define SRT_QUERY_SORT_ABI_VERSION 1" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(srt_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(NAMES) == sorted(_lib.QUERY_SORT_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", str(PKG / "libsrt_amd.so")], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [n for n in names if n not in exported]
    lib = _lib.lib()
    assert lib.srt_query_sort_abi_version() == 1
    # the additive header leaves the others alone
    assert lib.srt_query_abi_version() == 1 and lib.srt_rebuild_abi_version() == 1 and lib.srt_abi_version() == 2
    assert not set(_lib.QUERY_SORT_SYMBOLS) & set(_lib.QUERY_SYMBOLS)
    for n in names:
        assert isinstance(getattr(lib, n), C._CFuncPtr)


def test_the_rule_names_its_bit_counts_once():
    ob, db = rule_bits()
    assert 1 <= ob <= 10 and 0 <= db <= 10 and 3 * (ob + db) <= 32
    for f in ("ray_order_host.cpp", "query_sort.hpp", "query_sort.hip", "query.hip", "query.hpp"):
        assert "SRT_RAY_ORIGIN_BITS" not in (PKG / "csrc" / f).read_text()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4099])
def test_surface_style_rays_equal_the_restatement(surface_rays, n):
    rays = surface_rays[:n].copy()
    order, keys, box = check_against_restatement(rays)
    if n == 1:
        assert order[0] == 0 and (box[:3] == box[3:]).all()  # no extent: only the direction bits can be set
        assert keys[0] < (1 << 3 * rule_bits()[1])
    if n == 4099:
        assert len(np.unique(keys)) > 1000 and (order != np.arange(n)).any()
        assert (bits(box[:3]) == bits(rays["o"].min(0))).all() and (bits(box[3:]) == bits(rays["o"].max(0))).all()


def test_camera_rays_from_one_origin_differ_in_direction_bits_only():
    W, H = 96, 64
    x, y = np.meshgrid(np.arange(W, dtype=F), np.arange(H, dtype=F))
    rays = np.zeros(W * H, S.RAY_DTYPE)
    rays["o"] = (F(0.25), F(-3.0), F(7.5))
    rays["d"] = np.stack([(x.reshape(-1) - W / 2) / W, (y.reshape(-1) - H / 2) / H, np.full(W * H, -1.0)], 1).astype(F)
    rays["t"] = F(1e30)
    order, keys, box = check_against_restatement(rays)
    ob, db = rule_bits()
    assert (box[:3] == box[3:]).all() and (keys >> (3 * db) == 0).all()
    if db > 0:
        assert len(np.unique(keys)) > 1


def test_identical_rays_keep_their_order():
    rays = np.zeros(777, S.RAY_DTYPE)
    rays["o"], rays["d"], rays["t"] = (1.0, 2.0, 3.0), (0.5, -0.25, 1.0), F(9.0)
    order, keys, _ = check_against_restatement(rays)
    assert (order == np.arange(777)).all() and len(set(keys.tolist())) == 1


@pytest.mark.parametrize("family", ["special_values", "mixed_wave"])
def test_special_values_equal_the_restatement(rubik_scene, family):
    """NaN / Inf / 3e38 origins; zero, denormal, infinite and NaN directions."""
    rays, labels = getattr(SR, family)(rubik_scene)
    if family == "special_values":
        with np.errstate(invalid="ignore"):
            assert np.isnan(rays["o"]).any() and np.isinf(rays["o"]).any() and (rays["o"] == F(3e38)).any()
            assert np.isnan(rays["d"]).any() and np.isinf(rays["d"]).any() and (rays["d"] == 0).all(1).any()
    order, keys, box = check_against_restatement(rays)
    assert np.isfinite(box).all()
    if family == "special_values":
        assert (box[3:] == F(3e38)).all()  # finite, so part of the bounds


def test_signed_zeros_and_an_axis_without_a_finite_origin():
    rng = np.random.default_rng(5)
    rays = np.zeros(300, S.RAY_DTYPE)
    rays["o"] = rng.uniform(-2, 2, (300, 3)).astype(F)
    rays["d"] = rng.normal(size=(300, 3)).astype(F)
    rays["o"][:, 1] = np.resize(np.array([np.inf, -np.inf, np.nan], F), 300)   # y: no finite origin at all
    rays["o"][:, 2] = np.resize(np.array([0.0, -0.0, -0.0, 0.0], F), 300)       # z: lo is -0, hi is +0
    order, keys, box = check_against_restatement(rays)
    assert bits(box)[1] == 0 and bits(box)[4] == 0
    assert bits(box)[2] == 0x80000000 and bits(box)[5] == 0
    ob, db = rule_bits()
    y_bits = sum(1 << (3 * b + 1) for b in range(ob)) << (3 * db)
    z_bits = sum(1 << (3 * b) for b in range(ob)) << (3 * db)
    assert (keys & (y_bits | z_bits) == 0).all() and len(np.unique(keys)) > 50


def test_null_and_bad_arguments_without_a_device():
    lib = _lib.lib()
    buf = (C.c_uint8 * 256)()
    assert lib.srt_query_closest_sorted(None, None, 4, None) == _lib.SRT_ERR_INVALID
    assert lib.srt_query_occluded_sorted(None, None, 4, None) == _lib.SRT_ERR_INVALID
    assert lib.srt_query_closest_sorted(None, buf, 4, buf) == _lib.SRT_ERR_INVALID
    assert lib.srt_query_copy_ray_order(None, buf, buf, 4) == _lib.SRT_ERR_INVALID
    rays = np.zeros(4, S.RAY_DTYPE)
    out = np.full(4, 77, np.uint32)
    assert lib.srt_ray_order(None, 4, S._ptr(out), None, None) == _lib.SRT_ERR_INVALID
    assert lib.srt_ray_order(S._ptr(rays), 4, None, None, None) == _lib.SRT_ERR_INVALID
    assert (out == 77).all()
    assert lib.srt_ray_order(S._ptr(rays), 4, S._ptr(out), None, None) == _lib.SRT_OK and (out == np.arange(4)).all()
    box = np.full(6, 5.0, F)
    assert lib.srt_ray_order(None, 0, None, None, S._ptr(box)) == _lib.SRT_OK and (bits(box) == 0).all()
    order, keys = S.ray_order(np.zeros(0, S.RAY_DTYPE))
    assert len(order) == 0 and len(keys) == 0
    v = C.c_int()
    assert lib.srt_query_get_int(None, b"sort.bytes", C.byref(v)) == _lib.SRT_ERR_INVALID


def test_header_compiles_as_c(tmp_path):
    c = tmp_path / "t.c"
    c.write_text('#include "srt_query_sort.h"\n'
                 "int f(srt_query* q, const srt_ray* r, srt_hit* h, uint8_t* o, uint32_t* p, float* b) {\n"
                 "  return srt_query_sort_abi_version() + srt_query_closest_sorted(q, r, 1, h) +\n"
                 "         srt_query_occluded_sorted(q, r, 1, o) + srt_ray_order(r, 1, p, p, b) +\n"
                 "         srt_query_copy_ray_order(q, p, p, 1) + SRT_QUERY_SORT_ABI_VERSION;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", str(ROOT / "include"), str(c)], check=True)


def test_ray_order_host_under_sanitizers():
    """tests/cpp/test_ray_order_host.cpp with csrc/ray_order_host.cpp linked directly, AddressSanitizer + UBSan, as a
    stand-alone program (host code only: no HIP, no device, nothing preloaded)."""
    out = ROOT / "tests" / "cpp" / "_build"
    out.mkdir(exist_ok=True)
    exe = out / "test_ray_order_host_san"
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-ffp-contract=off", "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "cpp" / "test_ray_order_host.cpp"), str(PKG / "csrc" / "ray_order_host.cpp"),
                    "-o", str(exe), "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ray order host checks OK" in r.stdout


def test_cpp_mirror_compiles_and_orders_on_the_host(tmp_path):
    """include/srt/query.hpp: Query::ClosestSorted, Query::OccludedSorted and AssetUtils::RayOrder against the C ABI."""
    src = tmp_path / "m.cpp"
    src.write_text('#include <cstdio>\n#include <vector>\n#include "srt/query.hpp"\n'
                   "int main() {\n"
                   "  std::vector<srt_ray> rays(3);\n"
                   "  for (int i = 0; i < 3; ++i) { rays[i] = srt_ray{{float(2 - i), 0, 0}, 0, {0, 0, 1}, 1e30f}; }\n"
                   "  uint32_t order[3], keys[3]; float box[6];\n"
                   "  srt::AssetUtils::RayOrder(rays.data(), 3, order, keys, box);\n"
                   "  void (srt::Query::*a)(const srt_ray*, uint32_t, srt_hit*) = &srt::Query::ClosestSorted;\n"
                   "  void (srt::Query::*b)(const srt_ray*, uint32_t, uint8_t*) = &srt::Query::OccludedSorted;\n"
                   "  bool threw = false;\n"
                   "  try { srt::AssetUtils::RayOrder(nullptr, 3, order); } catch (const std::runtime_error&) { threw = true; }\n"
                   "  const bool ok = a && b && threw && order[0] == 2 && order[1] == 1 && order[2] == 0 && box[0] == 0 && box[3] == 2 &&\n"
                   "                  keys[0] <= keys[1] && keys[1] <= keys[2];\n"
                   '  std::printf(ok ? "ray order mirror OK\\n" : "ray order mirror FAILED\\n");\n'
                   "  return ok ? 0 : 1;\n}\n")
    exe = tmp_path / "m"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", str(ROOT / "include"), str(src), "-o", str(exe), "-L", str(PKG),
                    "-lsrt_amd", f"-Wl,-rpath,{PKG}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "ray order mirror OK" in r.stdout, r.stdout + r.stderr
