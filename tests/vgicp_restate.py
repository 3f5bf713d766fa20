"""Plain NumPy restatement of nanoPCL's voxelized GICP — registration::VoxelDistributionMap, VoxelCorrespondence::find and
alignVGICP (registration/voxel_distribution_map.hpp:143-323, correspondence/voxel_correspondence.hpp:35-78,
align.hpp:276-353) — written from the reference's sources and not from the engine: the reading fdm_voxel_map_create and
fdm_cloud_register_vgicp are held to (tests/test_vgicp_gpu.py); its own known answers are in tests/test_vgicp_restate.py.
Test data, not product.

The keys and runs are voxel_restate.sorted_runs (order 0: a voxel's points in input order); a voxel's sums are taken
SEQUENTIALLY in double, the first point assigned and the others added (step k adds the k-th point of every voxel that has
one: vectorised across voxels, never within one).  Records are in ascending key order and a correspondence names a
voxel by its rank in that order (this project's definition).  The regularised covariance of a voxel of three or more
points is reg_restate.regularize of the stored float32 covariance — in double, where the reference goes through float
(the documented DEVIATION, include/fdm_engine.h) — and the identity for a sparser one.  The factor, the sums and the loop
are reg_restate's GICP.
"""
import numpy as np

import reg_restate as RR
import voxel_restate as VR

F32 = np.float32
F64 = np.float64


class Map:
    """The voxel distribution map of (x, y, z) at `resolution`: key uint64[m] ascending, count uint32[m], mean
    float32[m, 3], cov float32[m, 3, 3] and creg float64[m, 3, 3] indexed [row][column], sums float64[m, 3] and outer
    float64[m, 3, 3] (what mean and cov were made of), n_skipped, gap float64[m] (the relative eigen-gap (l1 - l0) / l2 of
    cov, NaN for a sparse voxel)."""

    def __init__(self, x, y, z, resolution, eps=1e-3):
        x, y, z = (np.asarray(v, dtype=F32).reshape(-1) for v in (x, y, z))
        self.resolution, self.eps = F32(resolution), float(eps)
        self.inv = F32(1.0) / F32(resolution)
        sk, si, starts, counts = VR.sorted_runs(x, y, z, self.resolution, 0)
        m = starts.size
        self.n_points, self.n_skipped = x.size, x.size - sk.size
        self.key = sk[starts].astype(np.uint64) if m else np.zeros(0, dtype=np.uint64)
        self.count = counts.astype(np.uint32)
        p = np.stack([x[si], y[si], z[si]], axis=1).astype(F64)                   # sorted = input order within a voxel
        s = np.zeros((m, 3))
        o = np.zeros((m, 3, 3))
        if m:
            p0 = p[starts]
            s[:] = p0                                                             # assigned: a -0.0 stays -0.0
            o[:] = p0[:, :, None] * p0[:, None, :]
            for k in range(1, int(counts.max())):
                on = np.flatnonzero(counts > k)
                q = p[starts[on] + k]
                s[on] = s[on] + q
                o[on] = o[on] + q[:, :, None] * q[:, None, :]
        self.sums, self.outer = s, o
        cnt = counts.astype(F64)
        with np.errstate(over="ignore", invalid="ignore"):
            mean = s / cnt[:, None] if m else s
            self.mean = mean.astype(F32)
            cov = (o / cnt[:, None, None] - mean[:, :, None] * mean[:, None, :]).astype(F32) if m else o.astype(F32)
        full = counts >= 3
        cov[~full] = np.eye(3, dtype=F32) * F32(self.eps)
        self.cov = cov
        self.full = full
        self.creg = np.tile(np.eye(3), (m, 1, 1))
        if full.any():
            self.creg[full] = RR.regularize(cov[full], self.eps)
        self.gap = np.full(m, np.nan)
        for i in np.flatnonzero(full):
            a = cov[i].astype(F64)
            w = np.linalg.eigvalsh(np.tril(a) + np.tril(a, -1).T)
            self.gap[i] = (w[1] - w[0]) / w[2] if w[2] > 0 else 0.0

    @property
    def num_voxels(self):
        return self.key.size

    def min_gap(self):
        return float(np.nanmin(self.gap)) if self.full.any() else float("inf")

    def rank_of(self, p):
        """int64[n]: the rank of the voxel each point of p (float[n, 3], cast to float32) falls into, -1 for none."""
        q = np.asarray(p).astype(F32)
        if self.num_voxels == 0 or q.shape[0] == 0:
            return np.full(q.shape[0], -1, dtype=np.int64)
        _, key = VR.keys_of(q[:, 0], q[:, 1], q[:, 2], self.resolution)
        at = np.searchsorted(self.key, key)
        at = np.minimum(at, self.num_voxels - 1)
        return np.where(self.key[at] == key, at, -1).astype(np.int64)


class Problem:
    """A source cloud with covariances (float32[n, 3, 3] indexed [row][column]), a Map and the settings of one
    registration: the interface reg_restate.align expects.  max_correspondence_dist is carried and not used."""

    def __init__(self, source, source_cov, vmap, **settings):
        unknown = set(settings) - set(RR.DEFAULTS)
        assert not unknown, unknown
        self.set = dict(RR.DEFAULTS, **settings)
        if isinstance(self.set["robust_kernel"], str):
            self.set["robust_kernel"] = RR.KERNELS[self.set["robust_kernel"]]
        self.s = [np.asarray(v, dtype=F32).reshape(-1) for v in source]
        self.map = vmap
        self.t = [vmap.key]                                        # align's "empty target" test reads t[0].size
        self.source_cov = source_cov
        self.Cs = RR.regularize(source_cov, self.set["covariance_epsilon"])
        self.n = self.s[0].size

    def linearize(self, T, order="exact"):
        T = np.asarray(T, dtype=F64)
        p = RR.transform_points(T, *self.s)
        corr = self.map.rank_of(p)
        inl = np.flatnonzero(corr >= 0)
        j = corr[inl]
        S = RR.terms("gicp", p[inl], self.map.mean[j].astype(F64), self.set["robust_kernel"],
                     self.set["robust_kernel_width"], None, T[:3, :3], self.Cs[inl], self.map.creg[j])
        return {"sums": RR.column_sums(S, order), "abs_sums": RR.column_sums(np.abs(S), "exact"),
                "num_inliers": int(inl.size), "corr": corr, "terms": S}


def align(problem, initial_guess=None, order="forward"):
    return RR.align(problem, initial_guess, order)
