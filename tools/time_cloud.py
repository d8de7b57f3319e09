"""What scoring two clouds costs: the kernels of cloud.hip on their own, and a host k-d tree as the outside yardstick.

    python tools/time_cloud.py [--sizes 1000000x1000000,7700000x5000000] [--reps 10] [--timeout 600] [--no-host]

Clouds: NA queries and NB targets drawn (torch, seeded) on the sphere of radius 0.25 at the origin and moved along their normals by
N(0, 0.001) -- two independent samplings of one surface, in no spatial order, as two scans of one object are.  The box and the cell
size are diner_amd.cloudmetrics.grid_box's choice.  Each size runs in a child process of its own under --timeout seconds; a child that
fails ends the run.  Through the C entries on preallocated buffers, HIP events around each call, the median of --reps timed calls
after 3 warm-up calls:
  - diner_cloud_grid_build_f32 over the targets (and over the queries, which the own-order arrangement needs);
  - diner_cloud_nearest_f32 with the threads taking the queries in input order and in the cell order of the queries' own grid; the two
    outputs are compared bit for bit;
  - diner_cloud_reduce_f32 over the result.
The host yardstick, scipy.spatial.cKDTree(targets).query(queries, workers=16) in float64 when scipy imports, is timed once in the parent
(build and query apart) and its distances are compared with the kernel's.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RADIUS, SIGMA, SEED = 0.25, 0.001, 20261019


def sphere_cloud(n, seed, device):
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    u = torch.randn(n, 3, generator=g, dtype=torch.float64)
    u /= u.norm(dim=1, keepdim=True)
    return (u * (RADIUS + SIGMA * torch.randn(n, 1, generator=g, dtype=torch.float64))).to(torch.float32).to(device)


def child(args):
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    from diner_amd import _lib
    from diner_amd.cloudmetrics import grid_box
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    NA, NB = (int(v) for v in args.child.split("x"))
    a, b = sphere_cloud(NA, SEED, dev), sphere_cloud(NB, SEED + 1, dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def grid_of(xyz):
        lo, hi = xyz.amin(dim=0).cpu().tolist(), xyz.amax(dim=0).cpu().tolist()
        cell, dims = grid_box(lo, hi, xyz.shape[0])
        ws = torch.empty(lib.diner_cloud_grid_bytes(xyz.shape[0], *dims), dtype=torch.uint8, device=dev)
        return dict(xyz=xyz, n=int(xyz.shape[0]), lo=(C.c_float * 3)(*lo), cell=cell, dims=dims, ws=ws)

    def build(g):
        _lib.check(lib.diner_cloud_grid_build_f32(g["xyz"].data_ptr(), g["n"], g["lo"], g["cell"], *g["dims"], g["ws"].data_ptr(), st))

    def timed(fn):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        fn()
        ev1.record()
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1)

    def median_ms(fn, warm=3):
        for _ in range(warm):
            fn()
        return round(statistics.median(timed(fn) for _ in range(args.reps)), 4)

    gb, ga = grid_of(b), grid_of(a)
    res = dict(NA=NA, NB=NB, cell=gb["cell"], dims=list(gb["dims"]), grid_mib=round(gb["ws"].numel() / 2 ** 20, 1),
               build_targets_ms=median_ms(lambda: build(gb)), build_queries_ms=median_ms(lambda: build(ga)))
    at = lib.diner_cloud_grid_order_offset(NA, *ga["dims"])
    own = ga["ws"][at:at + 4 * NA].view(torch.int32).clone()
    outs = {k: (torch.empty(NA, device=dev), torch.empty(NA, dtype=torch.int32, device=dev)) for k in ("input", "own")}

    def nearest(kind):
        d2, idx = outs[kind]
        _lib.check(lib.diner_cloud_nearest_f32(b.data_ptr(), NB, gb["lo"], gb["cell"], *gb["dims"], gb["ws"].data_ptr(), a.data_ptr(), NA,
                                               own.data_ptr() if kind == "own" else None, float("inf"), d2.data_ptr(), idx.data_ptr(), st))

    # alternate the two arrangements, then take each one's median
    for kind in ("input", "own"):
        for _ in range(3):
            nearest(kind)
    times = {"input": [], "own": []}
    for _ in range(args.reps):
        for kind in ("input", "own"):
            times[kind].append(timed(lambda: nearest(kind)))
    res["nearest_input_order_ms"] = round(statistics.median(times["input"]), 4)
    res["nearest_own_order_ms"] = round(statistics.median(times["own"]), 4)
    res["same_bits"] = bool(torch.equal(outs["input"][0].view(torch.int32), outs["own"][0].view(torch.int32)) and
                            torch.equal(outs["input"][1], outs["own"][1]))
    res["queries_per_s_input_order"] = round(NA / (res["nearest_input_order_ms"] * 1e-3), -3)
    res["queries_per_s_own_order"] = round(NA / (res["nearest_own_order_ms"] * 1e-3), -3)
    d2, idx = outs["input"]
    rws = torch.empty(lib.diner_cloud_reduce_workspace_bytes(NA), dtype=torch.uint8, device=dev)
    out = torch.empty(11, dtype=torch.float64, device=dev)
    taus = (C.c_float * 8)(0.001, 0.002)
    res["reduce_ms"] = median_ms(lambda: _lib.check(lib.diner_cloud_reduce_f32(d2.data_ptr(), idx.data_ptr(), NA, float("inf"), taus, 2, None,
                                                                               None, 0, rws.data_ptr(), out.data_ptr(), st)))
    sums = out.cpu().tolist()
    res["matched"], res["mean_dist"] = int(sums[0]), sums[1] / max(sums[0], 1.0)
    if args.dump:
        import numpy as np
        np.save(args.dump, torch.sqrt(d2).cpu().numpy())
    print(json.dumps(res), flush=True)


def host_tree(NA, NB, dump):
    """scipy's k-d tree on the same clouds (float64): -> dict, or None when scipy does not import."""
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        return None
    import numpy as np
    a, b = sphere_cloud(NA, SEED, "cpu").numpy().astype(np.float64), sphere_cloud(NB, SEED + 1, "cpu").numpy().astype(np.float64)
    t0 = time.perf_counter()
    tree = cKDTree(b)
    t1 = time.perf_counter()
    d, _ = tree.query(a, workers=16)
    t2 = time.perf_counter()
    res = dict(build_ms=round((t1 - t0) * 1e3, 1), query_ms=round((t2 - t1) * 1e3, 1), workers=16)
    if dump and os.path.exists(dump):
        res["max_rel_diff_to_kernel"] = float(np.max(np.abs(np.load(dump).astype(np.float64) - d) / np.maximum(d, 1e-12)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000x1000000,7700000x5000000", help="NAxNB, comma-separated")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per child")
    ap.add_argument("--no-host", action="store_true", help="leave the host k-d tree out")
    ap.add_argument("--child", default="", help="(child) one NAxNB")
    ap.add_argument("--dump", default="", help="(child) write the distances here for the host comparison")
    args = ap.parse_args()
    if args.child:
        return child(args)
    import tempfile
    res = dict(tool="time_cloud", reps=args.reps, radius=RADIUS, sigma=SIGMA, runs={})
    with tempfile.TemporaryDirectory() as tmp:
        for size in args.sizes.split(","):
            dump = os.path.join(tmp, size + ".npy")
            cmd = [sys.executable, os.path.abspath(__file__), "--child", size, "--reps", str(args.reps)] + ([] if args.no_host else ["--dump", dump])
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"{size}: child exited with {p.returncode}")
            run = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            print(f"{size}: {run}", file=sys.stderr, flush=True)
            if not args.no_host:
                run["host_kd_tree"] = host_tree(run["NA"], run["NB"], dump)
                print(f"{size}: host {run['host_kd_tree']}", file=sys.stderr, flush=True)
            res["runs"][size] = run
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
