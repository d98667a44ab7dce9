"""The two walks of the fp64 plane product (csrc/plane.hip: plane_walk, VEXHIP_PLANE_WALK=0; plane_walk_ahead, 1 or unset) timed against
each other INSIDE one process, on one matrix and one pair of vectors: where x and y lie physically is worth 5 % of this product
(profiles/walk_header_ab.json: the same binary, 0.372 - 0.393 ms from process to process), more than what separates the walks.

    python tools/plane_walk_ab.py [--out FILE.json] [--shapes 512x384x384,...]

After 30 ms of launches: blocks of 50 products on device events, the switch flipped between blocks through vexhip_reload_env (the
product reads the library's snapshot of the environment at every launch), ten blocks per walk; a digest of y after every block.  Per
shape: the median of each walk, and as noise the spread (largest minus smallest block) of the parent walk.  The record is appended to
the list in FILE (one entry per process: run it in several processes to cover several placements)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch                                                     # noqa: E402

from vexcl_amd import lib, ops                                   # noqa: E402

BLOCKS, PRODUCTS = 10, 50


def set_walk(L, w):
    os.environ["VEXHIP_PLANE_WALK"] = str(w)
    L.reload_env()


def digest(y):
    v = y.view(torch.int64)
    return "%016x-%016x" % (int(v.sum().item()) & (2 ** 64 - 1), int((v ^ (v >> 17)).sum().item()) & (2 ** 64 - 1))


def block(step):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(PRODUCTS):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / PRODUCTS


def measure(L, A, x, y):
    step = lambda: A.apply(x, y, 1.0, False)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.030:                      # the device out of idle, both kernels loaded
        for w in (0, 1):
            set_walk(L, w)
            step()
        torch.cuda.synchronize()
    ms, sums = {0: [], 1: []}, {0: set(), 1: set()}
    for _ in range(BLOCKS):
        for w in (0, 1):
            set_walk(L, w)
            y.fill_(7.0)
            torch.cuda.synchronize()
            ms[w].append(block(step))
            sums[w].add(digest(y))
    med = {w: statistics.median(ms[w]) for w in (0, 1)}
    spread = max(ms[0]) - min(ms[0])
    return {"parent_walk_ms": round(med[0], 5), "new_walk_ms": round(med[1], 5), "parent_walk_spread_ms": round(spread, 5),
            "new_minus_parent_ms": round(med[1] - med[0], 5), "gain": round(1 - med[1] / med[0], 4),
            "faster_by_more_than_twice_the_spread": bool(med[0] - med[1] > 2 * spread),
            "within_spread_or_faster": bool(med[1] - med[0] <= spread),
            "parent_walk_blocks_ms": [round(v, 5) for v in ms[0]], "new_walk_blocks_ms": [round(v, 5) for v in ms[1]],
            "results_bit_identical": bool(len(sums[0] | sums[1]) == 1), "plane": dict(A.plane) if A.plane else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "plane_walk_ab.json"), help="the list of records this run is appended to")
    ap.add_argument("--shapes", default="512x384x384,512x384x768", help="grids of 512-point lines beside 512^3 (nx x ny x nz)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    L = lib()
    rows = {}
    n = 512
    ptr, col, val = ops.poisson3d(n, dev)
    x = ops.fill_hash(ops.device_vector(n ** 3, torch.float64, dev), 42)
    y = ops.device_vector(n ** 3, torch.float64, dev, zero=True)
    A = ops.SpMat(ptr, col, val)
    del ptr, col, val
    assert A.plane is not None and A.plane["tile"] == 2, A.plane
    rows["512^3"] = measure(L, A, x, y)
    rows["512^3"]["x_y_placement"] = [x.data_ptr() % (1 << 26), y.data_ptr() % (1 << 26)]
    print("512^3", json.dumps(rows["512^3"]), flush=True)
    del A, x, y
    torch.cuda.empty_cache()
    if args.shapes:
        from test_gpu_distributed import _stencil_strip
        for shape in args.shapes.split(","):
            nx, ny, nz = (int(v) for v in shape.split("x"))
            N = nx * ny * nz
            p, c, v = _stencil_strip(torch, nx, ny, nz, 0, N, dev)
            x = ops.fill_hash(ops.device_vector(N, torch.float64, dev), 7)
            y = ops.device_vector(N, torch.float64, dev, zero=True)
            A = ops.SpMat(p, c, v)
            del p, c, v
            if A.plane is None or A.plane["tile"] != 2 or A.plane["flat"]:
                rows[shape] = {"skipped": "not a plane plan with tiles of two", "plane": A.plane}
            else:
                rows[shape] = measure(L, A, x, y)
            print(shape, json.dumps(rows[shape]), flush=True)
            del A, x, y
            torch.cuda.empty_cache()
    os.environ.pop("VEXHIP_PLANE_WALK", None)
    L.reload_env()
    record = {"what": __doc__.split("\n\n")[2].replace("\n", " "), "device": torch.cuda.get_device_name(0), "blocks_per_walk": BLOCKS,
              "products_per_block": PRODUCTS, "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    runs = json.load(open(args.out)) if os.path.exists(args.out) else []
    runs.append(record)
    json.dump(runs, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
