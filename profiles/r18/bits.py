"""Every registration result as bytes: python profiles/r18/bits.py PACKAGE_ROOT OUT, from the repository root.  Cases and the oracle come from the
working tree; fastdem_amd from PACKAGE_ROOT."""
import os
import struct
import sys

root, out_path = os.path.abspath(sys.argv[1]), sys.argv[2]
REPO = os.getcwd()
sys.path[:0] = [root, os.path.join(REPO, "tests"), os.path.join(REPO, "oracle")]
import numpy as np   # noqa: E402
import torch   # noqa: E402
import fastdem_amd as F   # noqa: E402
assert os.path.abspath(F.__file__).startswith(root + os.sep), F.__file__
import reg_cases as RC   # noqa: E402
import reg_restate as RR   # noqa: E402
import vgicp_cases as VC   # noqa: E402

F32 = np.float32
lines = []


def dev(v):
    return None if v is None else torch.from_numpy(np.array(v, dtype=F32)).cuda()


def hx(a):
    return np.ascontiguousarray(np.asarray(a)).tobytes().hex()


def stats():
    st = F.register_last_stats()
    st.pop("ms")
    st["voxel"] = struct.pack("<f", st["voxel"]).hex()
    return repr(sorted(st.items()))


def put_align(label, r):
    lines.append(f"{label} T={hx(r.transform)} cov={'none' if r.covariance is None else hx(r.covariance)} "
                 f"rmse={struct.pack('<d', r.rmse).hex()} fitness={struct.pack('<d', r.fitness).hex()} "
                 f"it={r.iterations} conv={r.converged} stats={stats()}")


def put_lin(label, o):
    corr = o["corr"]
    if torch.is_tensor(corr):
        corr = corr.cpu().numpy()
    lines.append(f"{label} H={hx(o['H_upper'])} b={hx(o['b'])} err={struct.pack('<d', o['error']).hex()} "
                 f"n={o['num_inliers']} corr={hx(corr.astype(np.int32))} stats={stats()}")


for name in RC.ALIGN_CASES:
    case = RC.align_case(name)
    p = case.problem
    for on in (False, True):
        s, t, raw = list(p.s), list(p.t), dict(p.raw)
        if on:
            s, t, raw = [dev(v) for v in s], [dev(v) for v in t], {k: dev(v) for k, v in raw.items()}
        fn = {"icp": F.align_icp, "plane": F.align_plane_icp, "gicp": F.align_gicp}[p.method]
        extra = {"icp": (), "plane": (raw.get("target_normals"),), "gicp": (raw.get("source_cov"), raw.get("target_cov"))}[p.method]
        put_align(f"reg align {name} torch={on}", fn(*s, *t, *extra, initial_guess=case.guess, **dict(p.set)))

for name in VC.ALIGN_CASES:
    case = VC.align_case(name)
    for on in (False, True):
        s = [dev(v) for v in case.source] if on else list(case.source)
        cov = dev(case.source_cov) if on else case.source_cov
        tgt = [dev(v) for v in case.target] if on else list(case.target)
        with F.VoxelMap(*tgt, resolution=case.resolution,
                        covariance_epsilon=case.settings.get("covariance_epsilon", 1e-3)) as vm:
            put_align(f"vgicp align {name} map torch={on}", F.align_vgicp(*s, cov, voxel_map=vm, **case.settings))
        put_align(f"vgicp align {name} target torch={on}",
                  F.align_vgicp(*s, cov, target=tgt, voxel_resolution=case.resolution, **case.settings))

for method in ("icp", "plane", "gicp"):
    for kernel in (RR.NONE, RR.HUBER, RR.TUKEY, RR.CAUCHY):
        for ns, nt in ((1000, 1000), (257, 1000), (769, 257)):
            p = RC.lin_problem(method, kernel, ns, nt)
            for ti, T in enumerate(RC.lin_transforms()):
                for on in (False, True):
                    s, t, raw = list(p.s), list(p.t), dict(p.raw)
                    if on:
                        s, t, raw = [dev(v) for v in s], [dev(v) for v in t], {k: dev(v) for k, v in raw.items()}
                    put_lin(f"reg lin {method} k{kernel} {ns}x{nt} T{ti} torch={on}",
                            F.linearize(method, *s, *t, transform=T, return_correspondences=True, **raw, **dict(p.set)))

t_np, _, _ = VC.lin_base()
for kernel in (RR.NONE, RR.HUBER, RR.TUKEY, RR.CAUCHY):
    for ns in (257, 1000):
        p = VC.lin_problem(kernel, ns)
        for ti, T in enumerate(VC.lin_transforms()):
            for on in (False, True):
                s = [dev(v) for v in p.s] if on else list(p.s)
                cov = dev(p.source_cov) if on else p.source_cov
                tgt = [dev(v) for v in t_np] if on else list(t_np)
                with F.VoxelMap(*tgt, resolution=VC.EDGE) as vm:
                    put_lin(f"vgicp lin k{kernel} {ns} T{ti} map torch={on}",
                            F.linearize_vgicp(*s, cov, voxel_map=vm, transform=T, return_correspondences=True, **p.set))
                put_lin(f"vgicp lin k{kernel} {ns} T{ti} target torch={on}",
                        F.linearize_vgicp(*s, cov, target=tgt, voxel_resolution=VC.EDGE, transform=T,
                                          return_correspondences=True, **p.set))

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"{len(lines)} records -> {out_path}")
