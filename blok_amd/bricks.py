"""The sparse brick stream on the CPU (blok_bricks_*): the host build of HipTracer.volume_encode_bricks / volume_decode_bricks, and the
.bvol file that holds a stream.  A stream is the tuple (info, records, density payload, material payload): one _ffi.BRICKS_INFO record,
a structured array of _ffi.BRICK_RECORD, and two uint32 arrays (density bit patterns, material ids)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _ffi
from ._ffi import BlokError

FILLED_ONLY = _ffi.BRICKS_FILLED_ONLY
KEEP_OTHERS = _ffi.BRICKS_KEEP_OTHERS


def _vec(v):
    return None if v is None else (C.c_int32 * 3)(*[int(c) for c in v])


def _opt(a):
    return _ffi.ptr(a) if len(a) else None


def _stream(info, records, density_payload, material_payload):
    return (np.ascontiguousarray(info, dtype=_ffi.BRICKS_INFO).reshape(1), np.ascontiguousarray(records, dtype=_ffi.BRICK_RECORD).reshape(-1),
            np.ascontiguousarray(density_payload, dtype=np.uint32).reshape(-1), np.ascontiguousarray(material_payload, dtype=np.uint32).reshape(-1))


def encode_host(density, material_ids, origin=(0, 0, 0), lo=None, hi=None, flags: int = 0):
    """blok_bricks_encode over [z][y][x] arrays of a box at world `origin`; the region in world voxels, half open (both None = the whole
    box).  Two calls: the counts, then the arrays."""
    lib = _ffi.host_lib()
    d = np.ascontiguousarray(density, dtype=np.float32)
    m = np.ascontiguousarray(material_ids, dtype=np.uint32)
    assert d.ndim == 3 and m.shape == d.shape, "the arrays are [z][y][x] over the whole box"
    nz, ny, nx = d.shape
    info = np.zeros(1, dtype=_ffi.BRICKS_INFO)

    def call(records, dp, mp):
        rc = lib.blok_bricks_encode(_ffi.ptr(d), _ffi.ptr(m), _vec(origin), nx, ny, nz, _vec(lo), _vec(hi), int(flags), _ffi.ptr(info),
                                    None if records is None else _ffi.ptr(records), 0 if records is None else len(records),
                                    None if dp is None else _opt(dp), 0 if dp is None else len(dp),
                                    None if mp is None else _opt(mp), 0 if mp is None else len(mp))
        if rc != 0:
            raise BlokError(rc, "blok_bricks_encode")
    call(None, None, None)
    records = np.zeros(int(info["n_bricks"][0]), dtype=_ffi.BRICK_RECORD)
    dp = np.zeros(int(info["n_density"][0]), dtype=np.uint32)
    mp = np.zeros(int(info["n_material"][0]), dtype=np.uint32)
    if len(records):
        call(records, dp, mp)
    return info, records, dp, mp


def validate_host(info, records, density_payload, material_payload):
    """blok_bricks_validate: raises BlokError naming the rule and the first record that fails it."""
    info, records, dp, mp = _stream(info, records, density_payload, material_payload)
    err = C.create_string_buffer(256)
    rc = _ffi.host_lib().blok_bricks_validate(_ffi.ptr(info), _opt(records), _opt(dp), _opt(mp), err, len(err))
    if rc != 0:
        raise BlokError(rc, err.value.decode())


def decode_host(density, material_ids, origin, info, records, density_payload, material_payload, dst_lo=None, flags: int = 0):
    """blok_bricks_decode into the [z][y][x] arrays (contiguous float32 / uint32, written in place) of a box at world `origin`."""
    info, records, dp, mp = _stream(info, records, density_payload, material_payload)
    assert density.dtype == np.float32 and material_ids.dtype == np.uint32 and density.flags.c_contiguous and material_ids.flags.c_contiguous
    nz, ny, nx = density.shape
    err = C.create_string_buffer(256)
    rc = _ffi.host_lib().blok_bricks_decode(_ffi.ptr(density), _ffi.ptr(material_ids), _vec(origin), nx, ny, nz, _ffi.ptr(info), _opt(records),
                                            _opt(dp), _opt(mp), _vec(dst_lo), int(flags), err, len(err))
    if rc != 0:
        raise BlokError(rc, err.value.decode())


def write_file(path, info, records, density_payload, material_payload):
    info, records, dp, mp = _stream(info, records, density_payload, material_payload)
    err = C.create_string_buffer(512)
    rc = _ffi.host_lib().blok_bricks_write_file(os.fsencode(path), _ffi.ptr(info), _opt(records), _opt(dp), _opt(mp), err, len(err))
    if rc != 0:
        raise BlokError(rc, err.value.decode())


def read_file(path):
    """blok_bricks_read_file: the sizes first (checked against the file's length), then the arrays, validated."""
    lib = _ffi.host_lib()
    info = np.zeros(1, dtype=_ffi.BRICKS_INFO)
    err = C.create_string_buffer(512)
    rc = lib.blok_bricks_read_file(os.fsencode(path), _ffi.ptr(info), None, None, None, err, len(err))
    if rc != 0:
        raise BlokError(rc, err.value.decode())
    records = np.zeros(int(info["n_bricks"][0]), dtype=_ffi.BRICK_RECORD)
    dp = np.zeros(int(info["n_density"][0]), dtype=np.uint32)
    mp = np.zeros(int(info["n_material"][0]), dtype=np.uint32)
    if len(records) or len(dp) or len(mp):
        rc = lib.blok_bricks_read_file(os.fsencode(path), _ffi.ptr(info), _opt(records), _opt(dp), _opt(mp), err, len(err))
        if rc != 0:
            raise BlokError(rc, err.value.decode())
    return info, records, dp, mp
