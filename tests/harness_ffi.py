"""ctypes bindings for tests/host_harness/libhost_harness.so (the kernel body compiled for the CPU) — TESTS ONLY."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_harness"
LIB = SRC / "libhost_harness.so"
HIT = np.dtype([("t", "<f4"), ("material_id", "<u4"), ("voxel", "<i2", 3), ("face", "u1"), ("hit", "u1")])


def build(sanitize: bool = False, libm_pow: bool = False) -> Path:
    out = SRC / ("libhost_harness_asan.so" if sanitize else ("libhost_harness_libm_pow.so" if libm_pow else "libhost_harness.so"))
    deps = [SRC / "harness.cpp", SRC / "host_harness_shims.h", ROOT / "blok_amd/csrc/hip/trace_core.h",
            ROOT / "blok_amd/csrc/hip/path_core.h", ROOT / "blok_amd/csrc/hip/post_core.h",
            ROOT / "blok_amd/csrc/hip/trace_kernels.h", ROOT / "blok_amd/csrc/hip/tree_build.cpp",
            ROOT / "blok_amd/csrc/hip/tree.h"]
    if out.exists() and all(d.stat().st_mtime <= out.stat().st_mtime for d in deps):
        return out
    cmd = ["g++", "-O1", "-g", "-std=c++20", "-fPIC", "-ffp-contract=off", "-Wall", f"-I{ROOT / 'include'}",
           f"-I{ROOT / 'blok_amd/csrc/hip'}", f"-I{SRC}", "-shared", "-o", os.fspath(out),
           os.fspath(SRC / "harness.cpp"), os.fspath(ROOT / "blok_amd/csrc/hip/tree_build.cpp")]
    if sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]
    if libm_pow:
        cmd[1:1] = ["-DBLOK_PATH_LIBM_POW"]              # pow(x, 5 | 8 | 128) through libm, as the oracle writes them (path_core.h)
    subprocess.run(cmd, check=True)
    return out


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(os.fspath(build()))
        L.hh_build.restype = C.c_void_p
        L.hh_build.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_char_p)]
        L.hh_free.argtypes = [C.c_void_p]
        L.hh_levels.restype = C.c_uint32
        L.hh_levels.argtypes = [C.c_void_p]
        L.hh_voxels.restype = C.c_uint64
        L.hh_voxels.argtypes = [C.c_void_p]
        L.hh_trace_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.hh_trace_primary.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.hh_render_paths.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_uint32] * 6 + [C.c_void_p] * 4
        _lib = L
    return _lib


def render_paths_libm_pow(nodes, subs, cam, materials, width, height, spp=8, max_bounces=2, frame_index=0):
    """The path loop of the kernel body with the shader's three pow() calls through libm (the only operations in which the shipped body
    departs from the oracle's text): on one libm that build must equal the oracle bit for bit, colour included."""
    L = C.CDLL(os.fspath(build(libm_pow=True)))
    L.hh_build.restype = C.c_void_p
    L.hh_build.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_char_p)]
    L.hh_free.argtypes = [C.c_void_p]
    L.hh_render_paths.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_uint32] * 6 + [C.c_void_p] * 4
    why = C.c_char_p()
    h = L.hh_build(C.c_void_p(nodes.ctypes.data), len(nodes), C.c_void_p(subs.ctypes.data), len(subs), C.byref(why))
    if not h:
        raise RuntimeError(why.value.decode())
    materials = np.ascontiguousarray(materials)
    planes = {k: np.zeros((height, width, 4), dtype=np.float32) for k in ("color", "world_pos", "normal_roughness", "albedo_metallic")}
    L.hh_render_paths(C.c_void_p(h), C.c_void_p(cam.ctypes.data), C.c_void_p(materials.ctypes.data), len(materials), width, height, spp, max_bounces, frame_index,
                      *[C.c_void_p(planes[k].ctypes.data) for k in ("color", "world_pos", "normal_roughness", "albedo_metallic")])
    L.hh_free(C.c_void_p(h))
    return planes


class HostKernel:
    def __init__(self, nodes: np.ndarray, subs: np.ndarray):
        why = C.c_char_p()
        self.h = lib().hh_build(C.c_void_p(nodes.ctypes.data), len(nodes), C.c_void_p(subs.ctypes.data), len(subs),
                                C.byref(why))
        if not self.h:
            raise RuntimeError(why.value.decode())
        self.h = C.c_void_p(self.h)
        self.levels = lib().hh_levels(self.h)
        self.n_voxels = lib().hh_voxels(self.h)

    def __del__(self):
        if getattr(self, "h", None):
            lib().hh_free(self.h)
            self.h = None

    def tree_nodes(self):
        """(nodes as (n, 4) uint32, origin) of the host builder's tree (copies)."""
        L = lib()
        L.hh_tree_nodes.restype = C.c_void_p
        L.hh_tree_nodes.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]
        count, origin = C.c_size_t(), (C.c_int32 * 3)()
        p = L.hh_tree_nodes(self.h, C.byref(count), origin)
        buf = (C.c_char * (count.value * 16)).from_address(p)
        return np.frombuffer(buf, dtype=np.uint32).reshape(-1, 4).copy(), tuple(origin)

    def trace_rays(self, rays: np.ndarray) -> np.ndarray:
        out = np.zeros(len(rays), dtype=HIT)
        lib().hh_trace_rays(self.h, C.c_void_p(rays.ctypes.data), len(rays), C.c_void_p(out.ctypes.data))
        return out

    def trace_primary(self, cam: np.ndarray, width: int, height: int) -> np.ndarray:
        out = np.zeros(width * height, dtype=HIT)
        lib().hh_trace_primary(self.h, C.c_void_p(cam.ctypes.data), width, height, C.c_void_p(out.ctypes.data))
        return out


    def render_paths(self, cam, materials, width, height, spp=8, max_bounces=2, frame_index=0):
        materials = np.ascontiguousarray(materials)
        planes = {k: np.zeros((height, width, 4), dtype=np.float32)
                  for k in ("color", "world_pos", "normal_roughness", "albedo_metallic")}
        lib().hh_render_paths(self.h, C.c_void_p(cam.ctypes.data), C.c_void_p(materials.ctypes.data), len(materials),
                              width, height, spp, max_bounces, frame_index,
                              *[C.c_void_p(planes[k].ctypes.data) for k in ("color", "world_pos", "normal_roughness", "albedo_metallic")])
        return planes


# ---- the dense-grid kernel's body (blok_amd/csrc/hip/dense_core.h) through tests/host_harness/dense_shim.cpp ------------------------
def build_dense(sanitize: bool = False) -> Path:
    out = SRC / ("libdense_shim_asan.so" if sanitize else "libdense_shim.so")
    deps = [SRC / "dense_shim.cpp", SRC / "host_harness_shims.h", ROOT / "blok_amd/csrc/hip/dense_core.h",
            ROOT / "blok_amd/csrc/hip/trace_core.h", ROOT / "blok_amd/csrc/hip/trace_kernels.h", ROOT / "blok_amd/csrc/hip/tree.h"]
    if out.exists() and all(d.stat().st_mtime <= out.stat().st_mtime for d in deps):
        return out
    cmd = ["g++", "-O1", "-g", "-std=c++20", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", f"-I{ROOT / 'include'}",
           f"-I{ROOT / 'blok_amd/csrc/hip'}", f"-I{SRC}", "-shared", "-o", os.fspath(out), os.fspath(SRC / "dense_shim.cpp")]
    if sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]
    subprocess.run(cmd, check=True)
    return out


def load_dense(path) -> C.CDLL:
    L = C.CDLL(os.fspath(path))
    L.ds_new.restype = C.c_void_p
    L.ds_new.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    L.ds_free.argtypes = [C.c_void_p]
    L.ds_trace_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    L.ds_trace_primary.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p]
    L.ds_out_of_grid.restype = C.c_uint64
    L.ds_trace_steps.restype = C.c_uint32
    L.ds_trace_steps.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p]
    return L


_dense_lib = None


class HostDense:
    """ids[z][y][x] (0 = empty) at `origin`, tiled on the host; global_bits=True reads the occupancy words as the kernel does when
    they do not fit LDS (the global array), False as it does from its LDS copy.  lib: another build of the shim (the sanitizer one)."""

    def __init__(self, ids: np.ndarray, origin=(0, 0, 0), global_bits: bool = False, lib=None):
        global _dense_lib
        if lib is None:
            if _dense_lib is None:
                _dense_lib = load_dense(build_dense())
            lib = _dense_lib
        self.L = lib
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        nz, ny, nx = ids.shape
        o = np.asarray(origin, dtype=np.int32)
        self.global_bits = bool(global_bits)
        self.h = C.c_void_p(self.L.ds_new(C.c_void_p(ids.ctypes.data), nx, ny, nz, C.c_void_p(o.ctypes.data)))

    def __del__(self):
        if getattr(self, "h", None):
            self.L.ds_free(self.h)
            self.h = None

    def trace_rays(self, rays: np.ndarray) -> np.ndarray:
        rays = np.ascontiguousarray(rays)
        out = np.zeros(len(rays), dtype=HIT)
        self.L.ds_trace_rays(self.h, C.c_void_p(rays.ctypes.data), len(rays), int(self.global_bits), C.c_void_p(out.ctypes.data))
        self._inside()
        return out

    def _inside(self):
        n = self.L.ds_out_of_grid()
        if n:
            raise AssertionError(f"{n} walks addressed a tile outside the grid")

    def trace_steps(self, ray: np.ndarray, cap: int = 4096):
        """(record, axes of the steps in order) of one ray."""
        ray = np.ascontiguousarray(ray).reshape(1)
        out = np.zeros(1, dtype=HIT)
        steps = np.zeros(cap, dtype=np.uint8)
        n = self.L.ds_trace_steps(self.h, C.c_void_p(ray.ctypes.data), int(self.global_bits), C.c_void_p(steps.ctypes.data), cap, C.c_void_p(out.ctypes.data))
        self._inside()
        assert n <= cap
        return out[0], steps[:n]

    def trace_primary(self, cam: np.ndarray, width: int, height: int, jitter_clip=None) -> np.ndarray:
        cam = np.ascontiguousarray(cam)
        out = np.zeros(width * height, dtype=HIT)
        j = None if jitter_clip is None else np.asarray(jitter_clip, dtype=np.float32)
        self.L.ds_trace_primary(self.h, C.c_void_p(cam.ctypes.data), width, height, C.c_void_p(j.ctypes.data) if j is not None else None,
                                int(self.global_bits), C.c_void_p(out.ctypes.data))
        self._inside()
        return out
