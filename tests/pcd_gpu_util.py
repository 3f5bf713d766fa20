"""Helpers of the PCD GPU tests: where a file's data section is put before fdm_pcd_decode reads it, and the comparison
with the restatement (tests/pcd_restate.py)."""
import functools

import numpy as np

import pcd_restate as PR

CHANNELS = ("x", "y", "z", "intensity", "rgb", "nx", "ny", "nz")
# pageable host memory, pinned host memory (fdm_host_alloc) from the block's start and from inside it (read in place only on
# a 16-byte boundary), a device buffer at a 16-byte boundary and at base + k
PLACEMENTS = ["pageable", "pinned", "pinned+1", "pinned+16", "device+0", "device+1", "device+2", "device+3", "device+4", "device+7", "device+8"]


@functools.lru_cache(maxsize=None)
def restated(header, body):
    h = PR.parse_header(header)
    c = PR.load_body(h, body)
    for v in c.values():
        if v is not None:
            v.setflags(write=False)
    return c


def decode(gpu, header, body, placement="pageable", device=None):
    """fdm_pcd_decode of (header bytes, body bytes) with the body at `placement`; NumPy arrays either way."""
    import torch
    pcd = gpu.pcd
    h = pcd.parse_header(header)
    if placement == "pageable":
        out = pcd.decode(h, body, device)
    elif placement.startswith("pinned"):
        k = int(placement.split("+")[1]) if "+" in placement else 0
        host = gpu.HostArray(len(body) + k + 1, np.uint8)
        assert host.pinned
        host.array[k:k + len(body)] = np.frombuffer(body, dtype=np.uint8)
        out = pcd.decode(h, host.array[k:k + len(body)], device)
    else:
        k = int(placement.split("+")[1])
        buf = torch.zeros(len(body) + 64, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        buf[k:k + len(body)] = torch.frombuffer(bytearray(body), dtype=torch.uint8).cuda() if body else buf[:0]
        torch.cuda.synchronize()
        out = pcd.decode(h, None, device, body_ptr=buf.data_ptr() + k, body_bytes=len(body))
    if device is not None:
        out = {k: None if v is None else v.cpu().numpy().view(np.uint32 if k == "rgb" else np.float32) for k, v in out.items()}
    return out


def assert_same(got, want, what=""):
    """Bit for bit; a NaN on both sides counts as equal (F8 -> float conversions produce them)."""
    for k in CHANNELS:
        assert (got[k] is None) == (want[k] is None), (what, k)
        if want[k] is None:
            continue
        a, b = got[k].view(np.uint32), want[k].view(np.uint32)
        assert a.shape == b.shape, (what, k)
        same = a == b
        if k != "rgb":
            same |= np.isnan(got[k]) & np.isnan(want[k])
        bad = np.flatnonzero(~same)
        assert bad.size == 0, f"{what} {k}: {bad.size} differ, first {bad[:4]}: {a[bad[:4]]} != {b[bad[:4]]}"
