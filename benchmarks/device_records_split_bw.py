"""A batch of records that arrived in HBM split where it lies into its
columns (HBM -> HBM): gpu::DeviceSplitRecords (native.gpu.device_split_records,
route b), against
  (a) what a handler has without it: a D2H copy of the message, the host twin
      (native.pb_split_records), an H2D copy of every column and table;
  (c) gpu::DeviceBuildRecords on the same data, the way there;
  (d) the floor: ONE native.gpu.device_split_rows call with one job per ragged
      column, on per-column device_build_rows messages of the same values: the
      same payload bytes without the composition into one record.
Jobs: the builder benchmark's (benchmarks/device_records_bw.py): two columns
(int64 ids below 2^14 and float32 weights, the same row ends) and four (adding
a scalar int32 label per record and a ragged bytes blob). Shapes: 4 Ki, 64 Ki
and 1 Mi elements per ragged column as rows of 1, 32 and 1024 elements. The
receiver sizes the value arrays by the message alone and the row ends by the
record count, which travels with a batch (half the message's bytes, the bound
without it, makes a record table no arena block holds for the largest
shapes). Every call is timed on the host around the blocking call, warm-up
calls first, the median of --iters calls reported; the whole table is taken
--runs times and each figure printed with the range of the runs' medians. One
JSON line per shape.

  python benchmarks/device_records_split_bw.py [--elems 4096,...] [--iters 10] [--runs 3] [--routes a,b,c,d]
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

DTYPES = {0: np.int32, 3: np.int64, 7: np.uint8, 8: np.float32}


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
    ap.add_argument("--routes", default="a,b,c,d", help="b alone for a kernel trace of the splitter")
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
                msg = torch.empty(cap, dtype=torch.uint8, device=dev)
                build_job = [(4, table, rows, msg.data_ptr(), cap)]
                torch.cuda.synchronize()  # the uploads run on torch's stream, the codecs on theirs
                (length, err, _, _), = native.gpu.device_build_records(build_job, 0)
                assert err == 0, err
                if length > native.gpu.device_split_max_bytes():
                    continue
                # the receiver's outputs: values sized by the message, row ends by the record count
                outs, split_cols = [], []
                for inner, kind, t, ragged in cols:
                    width = t.element_size()
                    vals = torch.empty(length // (width if kind >= 8 else 1) if ragged else rows, dtype=t.dtype, device=dev)
                    out_ends = torch.empty(rows, dtype=torch.int32, device=dev) if ragged else None
                    outs.append((vals, out_ends))
                    split_cols.append((inner, kind, not ragged, vals.data_ptr(), vals.numel(),
                                       out_ends.data_ptr() if ragged else 0))
                split_job = [(4, split_cols, msg.data_ptr(), length, rows)]
                twin_cols = [(inner, kind, not ragged) for inner, kind, _, ragged in cols]
                # the floor: one rows message and one rows split job per ragged column
                row_jobs, keep = [], []
                for inner, kind, t, ragged in cols:
                    if not ragged:
                        continue
                    rcap = native.gpu.device_rows_worst_case(4, inner, kind, t.numel(), rows)
                    rmsg = torch.empty(rcap, dtype=torch.uint8, device=dev)
                    torch.cuda.synchronize()
                    (rlen, rerr, _), = native.gpu.device_build_rows(
                        [(4, inner, kind, t.data_ptr(), t.numel(), ends.data_ptr(), rows, rmsg.data_ptr(), rcap)], 0)
                    assert rerr == 0, rerr
                    rvals = torch.empty(rlen // (t.element_size() if kind >= 8 else 1), dtype=t.dtype, device=dev)
                    rends = torch.empty(rows, dtype=torch.int32, device=dev)
                    keep.append((rmsg, rvals, rends, t))
                    row_jobs.append((4, inner, kind, rmsg.data_ptr(), rlen, rvals.data_ptr(), rvals.numel(),
                                     rends.data_ptr(), rows))
                torch.cuda.synchronize()
                uploaded = []

                def split():
                    return native.gpu.device_split_records(split_job, 0)

                def baseline():
                    wire = msg[:length].cpu().numpy().tobytes()
                    got = native.pb_split_records(4, twin_cols, wire, rows, None, True)
                    assert got[0] == 0
                    up = []
                    for (inner, kind, _, ragged), (_, _, values, row_ends) in zip(cols, got[4]):
                        up.append(torch.from_numpy(np.frombuffer(values, dtype=DTYPES[kind])).to(dev))
                        up.append(torch.from_numpy(np.frombuffer(row_ends, dtype=np.int32)).to(dev) if ragged else None)
                    uploaded[:] = up
                    torch.cuda.synchronize()

                def build():
                    return native.gpu.device_build_records(build_job, 0)

                def floor():
                    return native.gpu.device_split_rows(row_jobs, 0)

                (nrows, _, err, _, counts), = split()
                assert (nrows, err) == (rows, 0), (nrows, err)
                baseline()
                for i, ((inner, kind, t, ragged), (vals, out_ends), (count, _)) in enumerate(zip(cols, outs, counts)):
                    assert count == t.numel() and torch.equal(vals[:count], t)  # the three paths give the columns back
                    assert torch.equal(uploaded[2 * i], t)
                    if ragged:
                        assert torch.equal(out_ends, ends) and torch.equal(uploaded[2 * i + 1], ends)
                for (count, nr, _, rerr, _), (_, rvals, rends, t) in zip(floor(), keep):
                    assert (count, nr, rerr) == (t.numel(), rows, 0) and torch.equal(rvals[:count], t)
                a, b, c, d = [], [], [], []
                for _ in range(args.runs):
                    if "b" in routes:
                        b.append(timed(split, args.warmup, args.iters) * 1e6)
                    if "a" in routes:
                        a.append(timed(baseline, 1, max(3, args.iters // 3)) * 1e6)
                    if "c" in routes:
                        c.append(timed(build, args.warmup, args.iters) * 1e6)
                    if "d" in routes:
                        d.append(timed(floor, args.warmup, args.iters) * 1e6)

                def col(x):
                    return {"median_us": round(statistics.median(x), 1), "min_us": round(min(x), 1),
                            "max_us": round(max(x), 1)} if x else None
                line = {"columns": ncols, "elements": n, "row_len": per, "rows": rows, "bytes": length,
                        "a_host_roundtrip": col(a), "b_device_split_records": col(b), "c_device_build_records": col(c),
                        "d_split_rows_per_column": col(d)}
                if a and b:
                    line["b_beats_a_every_run"] = all(y < x for x, y in zip(a, b))
                    line["a_over_b"] = round(statistics.median(a) / statistics.median(b), 2)
                if b and c:
                    line["b_over_c"] = round(statistics.median(b) / statistics.median(c), 2)
                if b and d:
                    line["b_over_d"] = round(statistics.median(b) / statistics.median(d), 2)
                print(json.dumps(line), flush=True)
    print(json.dumps({"device_codec_stats": native.gpu.device_codec_stats()}))


if __name__ == "__main__":
    main()
