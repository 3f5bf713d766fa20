#!/usr/bin/env python3
"""Cost of the PCD file path on the device, one JSON line per measurement:

  decode   device ms of k_pcd_decode at N points for 16-, 19- and 32-byte records, with the body at a 16-byte boundary
           of a device buffer and one byte behind it; beside it fdm_engine_ingest_cloud2 (k_ingest_count, k_pack_scan,
           k_ingest_write, one 4-byte download; torch events around the call) on the same blob for the one layout both
           accept: x y z intensity as F4, every point finite.  Run the script under `rocprofv3 --kernel-trace --stats`
           for k_ingest_write alone.
  pack     device ms of k_pcd_pack for 12- and 32-byte records at N points, beside fdm_engine_pack_cloud_device (torch
           events around the call) on a map with about as many valid cells.
  pcd2dem  wall time of fastdem_amd.pcd.pcd2dem on a binary file of N points, split into file read, build, export, file
           write; beside the route without this path: the file parsed in NumPy, build_dem from host arrays,
           to_point_cloud, the file written with NumPy; and the wall time of the build/pcd2dem binary, a process per run.

  python scripts/pcd_bench.py [--points 2100000] [--repeat 5] [--out profiles/pcd_bench.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_100_000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import fastdem_amd as F
    from fastdem_amd import capi, pcd
    lib = capi.load()
    lib.fdm_pcd_debug_profile(1)
    n, rep = args.points, args.repeat
    rng = np.random.default_rng(1)
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    def kernel_ms():
        ms = (C.c_float * 2)()
        lib.fdm_pcd_debug_last_kernel_ms(ms)
        return float(ms[0]), float(ms[1])

    def median(v):
        return float(np.median(v))

    # a campus-like cloud: 60 x 35 m of ground with noise, intensity and colour
    x = rng.uniform(-30, 30, n).astype(np.float32)
    y = rng.uniform(-17.5, 17.5, n).astype(np.float32)
    z = (0.05 * x + rng.normal(0, 0.02, n)).astype(np.float32)
    inten = rng.uniform(0, 1, n).astype(np.float32)
    rgb = rng.integers(0, 1 << 24, n).astype(np.uint32)
    cols = {"x": x.view(np.uint32), "y": y.view(np.uint32), "z": z.view(np.uint32), "intensity": inten.view(np.uint32),
            "rgb": rgb}

    def header(fields):
        return ("FIELDS " + " ".join(f[0] for f in fields) + "\nSIZE " + " ".join(str(f[2]) for f in fields) + "\nTYPE " +
                " ".join(f[1] for f in fields) + "\nCOUNT " + " ".join(str(f[3]) for f in fields) +
                f"\nWIDTH {n}\nHEIGHT 1\nPOINTS {n}\nDATA binary\n").encode()

    xyz = [("x", "F", 4, 1), ("y", "F", 4, 1), ("z", "F", 4, 1)]
    layouts = {
        16: (xyz + [("intensity", "F", 4, 1)], ["x", "y", "z", "intensity"], 0),
        19: (xyz + [("intensity", "F", 4, 1), ("ring", "U", 2, 1), ("flag", "U", 1, 1)], ["x", "y", "z", "intensity"], 3),
        32: (xyz + [("intensity", "F", 4, 1), ("rgb", "U", 4, 1), ("normal_x", "F", 4, 1), ("normal_y", "F", 4, 1),
                    ("normal_z", "F", 4, 1)], ["x", "y", "z", "intensity", "rgb", "x", "y", "z"], 0),
    }
    # ---- decode ----
    for size, (fields, names, tail) in layouts.items():
        rec = np.stack([cols[k] for k in names], 1).astype("<u4").view(np.uint8).reshape(n, 4 * len(names))
        if tail:
            rec = np.concatenate([rec, np.zeros((n, tail), np.uint8)], 1)
        assert rec.shape[1] == size
        h = pcd.parse_header(header(fields))
        buf = torch.zeros(n * size + 64, dtype=torch.uint8, device="cuda")
        host = torch.from_numpy(rec.reshape(-1))
        for shift in (0, 1):
            buf[shift:shift + n * size] = host.cuda()
            torch.cuda.synchronize()
            ms = []
            for _ in range(rep + 1):
                out = pcd.decode(h, None, 0, body_ptr=buf.data_ptr() + shift, body_bytes=n * size)
                ms.append(kernel_ms()[0])
            assert np.array_equal(out["x"].cpu().numpy(), x)
            emit(what="decode", kernel="k_pcd_decode", point_size=size, base_shift=shift, points=n, device_ms=median(ms[1:]),
                 gb_per_s=(n * size + 4 * n * sum(v is not None for v in out.values())) / median(ms[1:]) / 1e6)
        if size == 16:     # the PointCloud2 ingest on the same blob
            eng = F.Engine(10.0, 10.0, 0.5)
            lay = F.Engine.cloud2_layout(16, 0, 4, 8, intensity=12, intensity_type=7)
            buf[0:n * size] = host.cuda()
            torch.cuda.synchronize()
            nv = C.c_uint64(0)
            ms = []
            for _ in range(rep + 1):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                rc = lib.fdm_engine_ingest_cloud2(eng._h, C.c_void_p(buf.data_ptr()), 1, n, C.byref(lay), C.byref(nv))
                b.record()
                torch.cuda.synchronize()
                assert rc == 0 and nv.value == n
                ms.append(a.elapsed_time(b))
            emit(what="decode", kernel="fdm_engine_ingest_cloud2 (count + scan + write)", point_size=16, base_shift=0, points=n,
                 device_ms=median(ms[1:]))
            eng.close()
        del buf
    # ---- pack ----
    d = {k: torch.from_numpy(v.view(np.int32)).cuda() for k, v in cols.items()}
    fl = {k: (v if k == "rgb" else v.view(torch.float32)) for k, v in d.items()}
    for size, cloud in ((12, {"x": fl["x"], "y": fl["y"], "z": fl["z"]}),
                        (32, {"x": fl["x"], "y": fl["y"], "z": fl["z"], "intensity": fl["intensity"], "rgb": fl["rgb"],
                              "nx": fl["x"], "ny": fl["y"], "nz": fl["z"]})):
        ms = []
        for _ in range(rep + 1):
            body = pcd.encode(cloud)
            ms.append(kernel_ms()[1])
        assert len(body) == n * size
        emit(what="pack", kernel="k_pcd_pack", point_size=size, points=n, device_ms=median(ms[1:]),
             gb_per_s=2 * n * size / median(ms[1:]) / 1e6)
    side = int(np.sqrt(n)) + 1
    eng = F.Engine.create_map(side * 0.1, side * 0.1, 0.1)
    eng.set_layer("elevation", np.zeros((eng.rows, eng.cols), np.float32))      # every cell valid
    cells = eng.rows * eng.cols
    try:
        ms = []
        for _ in range(rep + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _, count, step = eng.pack_cloud_device()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        emit(what="pack", kernel="fdm_engine_pack_cloud_device (count + scan + write)", point_size=step, points=int(count),
             cells=cells, device_ms=median(ms[1:]))
    except Exception as e:  # noqa: BLE001  (a measurement script: say what could not be measured)
        emit(what="pack", kernel="fdm_engine_pack_cloud_device", error=str(e))
    eng.close()
    # ---- pcd2dem end to end ----
    fields, names, _ = layouts[16]
    rec = np.stack([cols[k] for k in names], 1).astype("<u4")
    with tempfile.TemporaryDirectory() as tmp:
        src, dst, dst2 = (os.path.join(tmp, f) for f in ("in.pcd", "out.pcd", "out_numpy.pcd"))
        with open(src, "wb") as f:
            f.write(header(fields))
            f.write(rec.tobytes())
        cfg = F.DEMConfig()
        for k in range(rep):
            t0 = time.perf_counter()
            with open(src, "rb") as f:
                data = f.read()
            t1 = time.perf_counter()
            eng = pcd.build_dem(data, cfg)
            t2 = time.perf_counter()
            body, cnt, hi, hc = eng.to_pcd()
            t3 = time.perf_counter()
            with open(dst, "wb") as f:
                f.write(pcd.write_header(cnt, hi, hc))
                f.write(body)
            t4 = time.perf_counter()
            eng.close()
            emit(what="pcd2dem", route="fdm_pcd_build_dem + fdm_engine_to_pcd", run=k, points=n, cells=int(cnt),
                 read_ms=(t1 - t0) * 1e3, build_ms=(t2 - t1) * 1e3, export_ms=(t3 - t2) * 1e3, write_ms=(t4 - t3) * 1e3,
                 total_ms=(t4 - t0) * 1e3)
        for k in range(rep):
            t0 = time.perf_counter()
            with open(src, "rb") as f:
                data = f.read()
            t1 = time.perf_counter()
            off = data.index(b"DATA binary\n") + 12
            a = np.frombuffer(data, dtype="<f4", offset=off, count=4 * n).reshape(n, 4)
            ch = [np.ascontiguousarray(a[:, q]) for q in range(4)]
            t2 = time.perf_counter()
            eng = F.build_dem(ch[0], ch[1], ch[2], ch[3], None, config=cfg)
            t3 = time.perf_counter()
            c = eng.to_point_cloud()
            out = np.stack([c["x"].view(np.uint32), c["y"].view(np.uint32), c["z"].view(np.uint32),
                            c["intensity"].view(np.uint32)], 1)
            t4 = time.perf_counter()
            with open(dst2, "wb") as f:
                f.write(pcd.write_header(len(out), True, False))
                f.write(out.tobytes())
            t5 = time.perf_counter()
            eng.close()
            emit(what="pcd2dem", route="NumPy parse + build_dem(host arrays) + to_point_cloud + NumPy write", run=k, points=n,
                 cells=len(out), read_ms=(t1 - t0) * 1e3, parse_ms=(t2 - t1) * 1e3, build_ms=(t3 - t2) * 1e3,
                 export_ms=(t4 - t3) * 1e3, write_ms=(t5 - t4) * 1e3, total_ms=(t5 - t0) * 1e3)
        with open(dst, "rb") as f1, open(dst2, "rb") as f2:
            emit(what="pcd2dem", same_output=f1.read() == f2.read())
        # the tool itself: a process of its own each time, so its wall time includes start-up and the device's
        tool = os.path.join(ROOT, "fastdem_amd", "cpp", "build", "pcd2dem")
        if os.path.exists(tool):
            import subprocess
            dst3 = os.path.join(tmp, "out_tool.pcd")
            for k in range(rep):
                t0 = time.perf_counter()
                r = subprocess.run([tool, src, dst3], capture_output=True, text=True)
                t1 = time.perf_counter()
                assert r.returncode == 0, r.stderr
                emit(what="pcd2dem", route="build/pcd2dem (one process per run)", run=k, points=n, total_ms=(t1 - t0) * 1e3)
            with open(dst, "rb") as f1, open(dst3, "rb") as f3:
                emit(what="pcd2dem", tool_same_output=f1.read() == f3.read())
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
