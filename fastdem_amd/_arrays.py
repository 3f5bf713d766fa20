"""Where a cloud call's arrays live: host NumPy arrays the library stages, or torch tensors it reads in place.

arrays(x, device) decides that once per call, from the first coordinate array, and this module is the only place in
the package that asks whether something is a tensor.  The contract every cloud entry point (cloud.py, pcd.py,
Engine.from_point_cloud, Engine.remove_floating_points) has through it:

1. A call is a tensor call iff `x` is a tensor.  Every other array argument must then be a tensor on the same device; in
   a NumPy call no argument may be a tensor.  Otherwise TypeError.
2. Tensors must live on a GPU (is_cuda); a CPU tensor raises TypeError.
3. Coordinate, intensity, normal and covariance tensors must be float32, rgb tensors int32 or uint32, index tensors any
   integer dtype (converted to 32 bits); another dtype raises TypeError.  NumPy arrays of any dtype are converted: the
   library stages them anyway.
4. Tensors are made contiguous.  Every prepared array is held by the adaptor, so it lives until the call returns.
5. The current stream of the tensors' device is synchronised before the call (and after an output is zero-filled), and
   the call runs on that device.  NumPy calls run on the caller's `device` argument.

Prepared inputs are flat (the library reads n, or 9 n, consecutive values).  Outputs are made where the inputs live;
index results are uint32 NumPy copies, or int64 tensors of the unsigned value.
"""
import ctypes as C

import numpy as np

_MIXED = "a call takes NumPy arrays throughout, or torch tensors that all live on the GPU of x throughout"


def _is_tensor(a):
    return hasattr(a, "data_ptr")


class _Arrays:
    """What the two backends share.  n: the size of x; device: the ordinal the call runs on; on_device: 0 or 1."""

    def _held(self, a):
        self._keep.append(a)
        return a

    def xyz(self, x, y, z):
        """The pointers of three coordinate arrays."""
        return [self.ptr(self.f32(v)) for v in (x, y, z)]

    def cloud5(self, x, y, z, intensity, rgb):
        """The pointers of x, y, z, intensity (or None) and rgb (or None)."""
        return self.xyz(x, y, z) + [self.ptr(self.f32(intensity)), self.ptr(self.u32(rgb))]

    def normals(self, v):
        """Normals given as three arrays or as one of shape (n, 3): the three prepared arrays (three None for None)."""
        if v is None:
            return (None,) * 3
        return tuple(self.f32(c) for c in (v if isinstance(v, (tuple, list)) else [v[:, k] for k in range(3)]))

    def cov_colmajor(self, cov, n):
        """n covariances indexed [row][column] (any shape of 9 n values) as the column-major array the library reads."""
        return None if cov is None else self._held(self.compact(self.f32(cov).reshape(n, 3, 3).swapaxes(1, 2)))

    def index_out(self, m):
        """A zero-filled index buffer of capacity max(m, 1); take(buffer, k) is the result of its first k entries."""
        return self.zeros(max(int(m), 1), "u32")


class _Host(_Arrays):
    on_device = 0
    _kinds = {"f32": np.float32, "u32": np.uint32, "i32": np.int32, "u8": np.uint8}

    def __init__(self, x, device):
        self.device, self.n, self._keep = int(device), int(np.size(x)), []

    def _prepared(self, v, dtype):
        if v is None:
            return None
        if _is_tensor(v):
            raise TypeError(_MIXED)
        return self._held(np.ascontiguousarray(v, dtype=dtype).reshape(-1))

    def f32(self, v):
        return self._prepared(v, np.float32)

    def u32(self, v):
        return self._prepared(v, np.uint32)

    def index(self, v):
        if v is not None and not _is_tensor(v):
            v = np.asarray(v).astype(np.uint32)       # (wraps like a C cast, whatever the integer dtype)
        return self._prepared(v, np.uint32)

    @staticmethod
    def ptr(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)

    def empty(self, shape, kind):
        """kind: "f32", "u32", "i32", "u8", or a prepared array whose dtype the output shares."""
        return np.empty(shape, dtype=kind.dtype if hasattr(kind, "dtype") else self._kinds[kind])

    def zeros(self, shape, kind):
        return np.zeros(shape, dtype=self._kinds[kind])

    compact = staticmethod(np.ascontiguousarray)

    @staticmethod
    def take(a, k):
        return a[:k].copy()

    @staticmethod
    def mask(keep8):
        """The keep mask a call returns, of the uint8 array the library filled."""
        return keep8.astype(bool)


class _Device(_Arrays):
    on_device = 1

    def __init__(self, where, n):
        import torch
        self._torch, self._where, self.n, self._keep = torch, where, n, []
        self._kinds = {"f32": torch.float32, "u32": torch.int32, "i32": torch.int32, "u8": torch.uint8}
        self.device = where.index if where.index is not None else torch.cuda.current_device()
        self.sync()

    def sync(self):
        self._torch.cuda.current_stream(self._where).synchronize()

    def _made(self, new, of):
        if new.data_ptr() != of.data_ptr():
            self.sync()                               # a copy, made on torch's stream: complete before the library reads it
        return new

    def _prepared(self, v, dtypes, convert=lambda t: t):
        if v is None:
            return None
        if not _is_tensor(v) or v.device != self._where:
            raise TypeError(_MIXED)
        if v.dtype not in dtypes:
            raise TypeError(f"a {v.dtype} tensor where one of {dtypes} is taken")
        return self._held(self._made(convert(v).contiguous().view(-1), v))

    def f32(self, v):
        return self._prepared(v, (self._torch.float32,))

    def u32(self, v):
        return self._prepared(v, (self._torch.int32, self._torch.uint32))

    def index(self, v):
        t = self._torch
        return self._prepared(v, (t.uint8, t.int8, t.int16, t.int32, t.int64, t.uint16, t.uint32, t.uint64),
                              lambda a: a.to(t.int64).to(t.int32))

    @staticmethod
    def ptr(a):
        return None if a is None else C.c_void_p(a.data_ptr())

    def empty(self, shape, kind):
        return self._torch.empty(shape, dtype=kind.dtype if hasattr(kind, "dtype") else self._kinds[kind], device=self._where)

    def zeros(self, shape, kind):
        a = self._torch.zeros(shape, dtype=self._kinds[kind], device=self._where)
        self.sync()                                   # the library writes on a stream of its own
        return a

    def compact(self, a):
        return self._made(a.contiguous(), a)

    @staticmethod
    def take(a, k):
        return a[:k].long() & 0xFFFFFFFF

    @staticmethod
    def mask(keep8):
        return keep8


def arrays(x, device=0):
    """The adaptor of a call whose first coordinate array is x; `device`: the ordinal a NumPy call runs on."""
    if not _is_tensor(x):
        return _Host(x, device)
    if not x.is_cuda:
        raise TypeError("a torch tensor must live on a GPU; pass host data as NumPy arrays")
    return _Device(x.device, x.numel())


def outputs(device):
    """The adaptor of a call without array inputs: NumPy outputs for device None, tensors on that ordinal otherwise."""
    if device is None:
        return _Host((), 0)
    import torch
    return _Device(torch.device("cuda", int(device)), 0)


def complement(indices, total):
    """The indices 0 .. total - 1 that are not in `indices`, ascending, where `indices` lives."""
    if _is_tensor(indices):
        import torch
        mask = torch.ones(int(total), dtype=torch.bool, device=indices.device)
        mask[indices] = False
        return torch.nonzero(mask).reshape(-1)
    mask = np.ones(int(total), dtype=bool)
    mask[indices] = False
    return np.nonzero(mask)[0].astype(np.uint32)


def to_numpy(a):
    """A NumPy array of a result, wherever it lives."""
    return a.cpu().numpy() if _is_tensor(a) else np.asarray(a)
