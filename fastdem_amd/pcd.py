"""PCD files over the C ABI (include/fdm_engine.h, the fdm_pcd_* block): nanopcl::io::loadPCD / savePCD and the pcd2dem
tool (fastdem/tools/pcd2dem.cpp).  Plumbing only: the header and ASCII records are parsed by the library on the host,
binary records are decoded and packed by its kernels.
"""
import ctypes as C

import numpy as np

from . import capi
from .capi import FdmDemStats, FdmPcdHeader
from ._arrays import arrays, outputs
from .cloud import DEMConfig
from .engine import Engine, _ck, _ptr

ASCII, BINARY = capi.PCD_ASCII, capi.PCD_BINARY
CHANNELS = ("x", "y", "z", "intensity", "rgb", "nx", "ny", "nz")


def parse_header(data):
    """parseHeader over the first bytes of a file: the fdm_pcd_header (fields, width, height, point_size, viewpoint,
    format, data_offset, the chosen field indices).  Raises EngineError where the reference throws."""
    data = bytes(data)
    h = FdmPcdHeader()
    _ck(capi.load().fdm_pcd_parse_header(data, len(data), C.byref(h)))
    return h


def write_header(n, has_intensity=False, has_rgb=False, has_normal=False, viewpoint=None, fmt=BINARY):
    """savePCD's header text, as bytes; viewpoint = (tx, ty, tz, qw, qx, qy, qz) or None for the identity."""
    lib = capi.load()
    vp = None if viewpoint is None else (C.c_double * 7)(*[float(v) for v in viewpoint])
    buf = C.create_string_buffer(512)
    need = C.c_uint64(0)
    rc = _ck(lib.fdm_pcd_write_header(int(n), int(has_intensity), int(has_rgb), int(has_normal), vp, int(fmt), buf, 512,
                                      C.byref(need)))
    assert rc == 0, rc
    return buf.raw[:need.value]


def present(h):
    """Which of CHANNELS a file with header h has."""
    idx = dict(zip(CHANNELS, (h.idx_x, h.idx_y, h.idx_z, h.idx_intensity, h.idx_rgb, h.idx_nx, h.idx_ny, h.idx_nz)))
    normal = idx["nx"] >= 0 and idx["ny"] >= 0 and idx["nz"] >= 0
    return {k: (v >= 0 and (normal or k not in ("nx", "ny", "nz"))) for k, v in idx.items()}


def decode(h, body, device=None, body_ptr=None, body_bytes=None):
    """loadPCD's data section.  body: bytes-like (host), or with body_ptr / body_bytes a device pointer.  device None:
    dict of NumPy arrays; an ordinal: dict of torch tensors on that device.  Channels the file lacks are None."""
    lib = capi.load()
    n = (h.width * h.height) & 0xFFFFFFFF
    has = present(h) if n else dict.fromkeys(CHANNELS, False)
    for k in "xyz":
        has[k] = True
    A = outputs(device)
    out = {k: A.zeros(n, "u32" if k == "rgb" else "f32") if has[k] else None for k in CHANNELS}
    if body_ptr is not None:
        src, size, on_device = C.c_void_p(body_ptr), int(body_bytes), 1
    else:
        keep = np.frombuffer(body, dtype=np.uint8)
        src, size, on_device = _ptr(keep) if keep.size else None, keep.size, 0
    _ck(lib.fdm_pcd_decode(C.byref(h), src, size, on_device, *[A.ptr(out[k]) for k in CHANNELS], A.on_device, A.device))
    return out


def load_pcd(path, device=None, return_header=False):
    """nanopcl::io::loadPCD(path): dict x, y, z, intensity, rgb (0x00RRGGBB), nx, ny, nz — NumPy arrays, or torch tensors
    on `device`; None for a channel the file lacks."""
    with open(path, "rb") as f:
        data = f.read()
    h = parse_header(data)
    cloud = decode(h, memoryview(data)[h.data_offset:], device)
    return (cloud, h) if return_header else cloud


def encode(cloud, fmt=BINARY, precision=8, device=0):
    """savePCD's data section for a dict of NumPy arrays or torch device tensors (absent channels None or missing)."""
    lib = capi.load()
    A = arrays(cloud["x"], device)
    vals = [A.u32(cloud.get(k)) if k == "rgb" else A.f32(cloud.get(k)) for k in CHANNELS]
    n = A.n
    call = (n, *[A.ptr(v) for v in vals], A.on_device, int(fmt), int(precision), A.device)
    need = C.c_uint64(0)
    words = sum(v is not None for v in vals)
    cap = n * words * 4 if fmt == BINARY else 0
    buf = np.empty(max(cap, 1), dtype=np.uint8)
    rc = _ck(lib.fdm_pcd_encode(*call, _ptr(buf), cap, C.byref(need)))
    if rc == capi.FDM_SKIP_BUFFER_TOO_SMALL:                  # ASCII: the size is known once the text exists
        cap = need.value
        buf = np.empty(max(cap, 1), dtype=np.uint8)
        rc = _ck(lib.fdm_pcd_encode(*call, _ptr(buf), cap, C.byref(need)))
    assert rc == 0, rc
    return buf[:need.value].tobytes()


def save_pcd(path, cloud, fmt=BINARY, precision=8, viewpoint=None, device=0):
    """nanopcl::io::savePCD(path, cloud, options)."""
    has = {k: cloud.get(k) is not None for k in CHANNELS}
    n = arrays(cloud["x"], device).n
    head = write_header(n, has["intensity"], has["rgb"], has["nx"] and has["ny"] and has["nz"], viewpoint, fmt)
    body = encode(cloud, fmt, precision, device)
    with open(path, "wb") as f:
        f.write(head)
        f.write(body)


def build_dem(data, config=None, device=0, return_stats=False):
    """buildDEM(loadPCD(file), config) for a file's bytes: a map-only Engine, or None where the reference returns an
    uninitialised map.  return_stats: (engine, status)."""
    lib = capi.load()
    h = parse_header(data)
    body = np.frombuffer(memoryview(data)[h.data_offset:], dtype=np.uint8)
    cfg = (config if config is not None else DEMConfig()).as_struct()
    handle, st = C.c_void_p(), FdmDemStats()
    rc = _ck(lib.fdm_pcd_build_dem(C.byref(h), _ptr(body) if body.size else None, body.size, 0, C.byref(cfg), int(device),
                                   C.byref(handle), C.byref(st)))
    eng = Engine._adopt(handle) if rc == 0 and handle.value else None
    return (eng, rc) if return_stats else eng


def pcd2dem(src, dst, config=None, device=0):
    """The pcd2dem tool: loadPCD(src) -> buildDEM -> toPointCloud -> savePCD(dst).  Returns the number of elevation cells
    written.  A cloud that leaves no map (an empty or fully filtered one) gives a file of 0 points, as build/pcd2dem
    writes it."""
    with open(src, "rb") as f:
        data = f.read()
    eng = build_dem(data, config, device)
    body, n, hi, hc = b"", 0, False, False
    if eng is not None:
        try:
            body, n, hi, hc = eng.to_pcd()
        finally:
            eng.close()
    with open(dst, "wb") as f:
        f.write(write_header(n, hi, hc, False, None, BINARY))
        f.write(body)
    return n
