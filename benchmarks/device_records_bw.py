"""A batch of records serialized where it lives (HBM -> HBM) as the
occurrences of one repeated sub-message with several fields:
gpu::DeviceBuildRecords (native.gpu.device_build_records), against
  (a) what a handler had before it: D2H copies of every column and table,
      the host twin (native.pb_serialize_records), an H2D copy of the bytes;
  (c) the floor: ONE native.gpu.device_build_rows call with one job per
      ragged column on the same data, the same payload bytes without the
      composition into one sub-message per record.
Jobs: two columns (int64 ids below 2^14: 2-byte varints, and float32 weights,
the same row ends) and four (adding a scalar int32 label per record and a
ragged bytes blob). Shapes: 4 Ki, 64 Ki and 1 Mi elements per ragged column as
rows of 1, 32 and 1024 elements. Every call is timed on the host around the
blocking call (the builders wait for their stream, the baseline ends in a
device synchronize), warm-up calls first, the median of --iters calls
reported; the whole table is taken --runs times and each figure printed with
the range of the runs' medians. One JSON line per shape.

  python benchmarks/device_records_bw.py [--elems 4096,...] [--iters 10] [--runs 3] [--routes a,b,c]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(call, warmup, iters):
    for _ in range(warmup):
        call()
    out = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        out.append(time.perf_counter() - t0)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elems", default="4096,65536,1048576")
    ap.add_argument("--row-lens", default="1,32,1024")
    ap.add_argument("--columns", default="2,4")
    ap.add_argument("--routes", default="a,b,c", help="b alone for a kernel trace of the builder")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    routes = args.routes.split(",")
    from brpc_amd import native
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is no CPU figure"
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    for ncols in [int(x) for x in args.columns.split(",")]:
        for n in [int(x) for x in args.elems.split(",")]:
            ids = torch.from_numpy(rng.integers(1 << 7, 1 << 14, n).astype(np.int64)).to(dev)
            weights = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dev)
            blob = torch.from_numpy(rng.integers(0, 256, n).astype(np.uint8)).to(dev)
            for per in [int(x) for x in args.row_lens.split(",")]:
                ends_np = np.arange(per, n + 1, per, dtype=np.uint32)
                if ends_np.size == 0 or ends_np[-1] != n:
                    ends_np = np.append(ends_np, np.uint32(n))
                ends = torch.from_numpy(ends_np.view(np.int32).copy()).to(dev)
                rows = int(ends_np.size)
                label = torch.from_numpy(rng.integers(-3, 100, rows).astype(np.int32)).to(dev)
                # (inner, kind, tensor, ragged)
                cols = [(1, 3, ids, True), (2, 8, weights, True)]
                if ncols == 4:
                    cols += [(3, 0, label, False), (4, 7, blob, True)]
                table = [(inner, kind, t.data_ptr(), t.numel(), ends.data_ptr() if ragged else 0)
                         for inner, kind, t, ragged in cols]
                cap = native.gpu.device_records_worst_case(4, table, rows)
                dst = torch.empty(cap, dtype=torch.uint8, device=dev)
                job = [(4, table, rows, dst.data_ptr(), cap)]
                row_jobs, row_dsts = [], []
                for inner, kind, t, ragged in cols:
                    if not ragged:
                        continue
                    rcap = native.gpu.device_rows_worst_case(4, inner, kind, t.numel(), rows)
                    row_dsts.append(torch.empty(rcap, dtype=torch.uint8, device=dev))
                    row_jobs.append((4, inner, kind, t.data_ptr(), t.numel(), ends.data_ptr(), rows,
                                     row_dsts[-1].data_ptr(), rcap))
                torch.cuda.synchronize()  # the uploads run on torch's stream, the builders on theirs
                uploaded = []

                def build():
                    return native.gpu.device_build_records(job, 0)

                def baseline():
                    host_ends = ends.cpu().numpy().tobytes()
                    host_cols = [(inner, kind, t.cpu().numpy().tobytes(), host_ends if ragged else None)
                                 for inner, kind, t, ragged in cols]
                    err, _, _, wire = native.pb_serialize_records(4, host_cols, rows)
                    uploaded[:] = [torch.frombuffer(bytearray(wire), dtype=torch.uint8).to(dev)]
                    torch.cuda.synchronize()

                def floor():
                    return native.gpu.device_build_rows(row_jobs, 0)

                (length, err, _, _), = build()
                assert err == 0, err
                baseline()
                assert torch.equal(dst[:length], uploaded[0])  # the two paths make the same bytes
                assert all(r[1] == 0 for r in floor())
                a, b, c = [], [], []
                for _ in range(args.runs):
                    if "b" in routes:
                        b.append(timed(build, args.warmup, args.iters) * 1e6)
                    if "a" in routes:
                        a.append(timed(baseline, args.warmup, args.iters) * 1e6)
                    if "c" in routes:
                        c.append(timed(floor, args.warmup, args.iters) * 1e6)

                def col(x):
                    return {"median_us": round(statistics.median(x), 1), "min_us": round(min(x), 1),
                            "max_us": round(max(x), 1)} if x else None
                line = {"columns": ncols, "elements": n, "row_len": per, "rows": rows, "bytes": length,
                        "a_host_roundtrip": col(a), "b_device_records": col(b), "c_rows_per_column": col(c)}
                if a and b:
                    line["b_wins_every_run"] = all(y < x for x, y in zip(a, b))
                    line["a_over_b"] = round(statistics.median(a) / statistics.median(b), 2)
                if b and c:
                    line["b_over_c"] = round(statistics.median(b) / statistics.median(c), 2)
                print(json.dumps(line), flush=True)
    print(json.dumps({"device_codec_stats": native.gpu.device_codec_stats()}))


if __name__ == "__main__":
    main()
