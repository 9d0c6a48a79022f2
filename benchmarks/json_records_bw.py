"""Columns of a batch that lie in HBM printed as a JSON array of objects where
they lie (HBM -> HBM): gpu::DevicePrintRecordObjects
(native.gpu.device_json_print_records, route b), against
  (a) what a handler has without it: a D2H copy of every column and table, the
      host twin (native.json_format_record_objects), an H2D copy of the text;
  (c) the floor: the same payload bytes without the composition into objects,
      one call of the per-column printer per column (device_json_print_numbers,
      device_json_escape with row ends, device_base64_encode_rows).
Jobs: the data of benchmarks/device_records_split_bw.py: two columns (int64 ids
below 2^14 and float32 weights, the same row ends) and four (adding a scalar
int32 label per record and a ragged blob, printed once as a string and once as
base64). Shapes: 4 Ki, 64 Ki and 1 Mi elements per ragged column as rows of 1,
32 and 1024 elements. Every call is timed on the host around the blocking
call, warm-up calls first, the median of --iters calls reported; the whole
table is taken --runs times and each figure printed with the range of the
runs' medians. One JSON line per shape.

  python benchmarks/json_records_bw.py [--elems 4096,...] [--iters 10] [--runs 3] [--routes a,b,c]
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

NUMBER, STRING, BASE64 = 0, 1, 2


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
    ap.add_argument("--columns", default="2,4s,4b", help="2: ids and weights; 4s / 4b: plus a label and a blob as "
                                                          "string / base64")
    ap.add_argument("--routes", default="a,b,c", help="b alone for a kernel trace of the printer")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    routes = args.routes.split(",")
    from brpc_amd import native
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is no CPU figure"
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    for shape in args.columns.split(","):
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
                # (key, kind, text form, tensor, ragged)
                cols = [(b"input_ids", 3, NUMBER, ids, True), (b"weights", 8, NUMBER, weights, True)]
                if shape != "2":
                    cols += [(b"label", 0, NUMBER, label, False),
                             (b"blob", 7, STRING if shape == "4s" else BASE64, blob, True)]
                table = [(key, kind, text, t.data_ptr(), t.numel(), ends.data_ptr() if ragged else 0)
                         for key, kind, text, t, ragged in cols]
                cap = native.gpu.json_records_worst_case(table, rows, True)
                out = torch.empty(cap, dtype=torch.uint8, device=dev)
                job = [(table, rows, True, out.data_ptr(), cap)]
                # the floor: one job of the column's own printer per column, each call by itself
                # (function, arguments, where its result keeps the code)
                floor_calls, keep = [], []
                for key, kind, text, t, ragged in cols:
                    if text == NUMBER:
                        fcap = native.gpu.json_number_print_worst_case(kind, t.numel(), rows if ragged else 0)
                        fout = torch.empty(fcap, dtype=torch.uint8, device=dev)
                        fargs = ([t.data_ptr()], [t.numel()], [kind], [ends.data_ptr() if ragged else 0],
                                 [rows if ragged else 0], [True], [fout.data_ptr()], [fcap], 0)
                        floor_calls.append((native.gpu.device_json_print_numbers, fargs, 2))
                    elif text == STRING:
                        fcap = native.gpu.json_escape_worst_case(t.numel(), rows)
                        fout = torch.empty(fcap, dtype=torch.uint8, device=dev)
                        fargs = ([t.data_ptr()], [t.numel()], [fout.data_ptr()], [fcap], [ends.data_ptr()], [rows], True, 0)
                        floor_calls.append((native.gpu.device_json_escape, fargs, 1))
                    else:
                        fcap = native.gpu.base64_rows_worst_case(t.numel(), rows, True)
                        fout = torch.empty(fcap, dtype=torch.uint8, device=dev)
                        fargs = ([t.data_ptr()], [t.numel()], [ends.data_ptr()], [rows], True, [fout.data_ptr()], [fcap], 0)
                        floor_calls.append((native.gpu.device_base64_encode_rows, fargs, 1))
                    keep.append(fout)
                torch.cuda.synchronize()  # the uploads run on torch's stream, the printers on theirs
                uploaded = []

                def device():
                    return native.gpu.device_json_print_records(job, 0)

                def baseline():
                    twin = [(key, kind, text, t.cpu().numpy().tobytes(), ends.cpu().numpy().tobytes() if ragged else None)
                            for key, kind, text, t, ragged in cols]
                    err, _, _, host_text = native.json_format_record_objects(twin, rows, True)
                    assert err == 0
                    uploaded[:] = [torch.from_numpy(np.frombuffer(host_text, dtype=np.uint8)).to(dev)]
                    torch.cuda.synchronize()

                def floor():
                    return [fn(*fargs)[0][at] for fn, fargs, at in floor_calls]

                (length, err, _, _), = device()
                assert err == 0, err
                baseline()
                assert torch.equal(out[:length], uploaded[0])  # both routes print the same bytes
                assert not any(floor()), floor()
                a, b, c = [], [], []
                for _ in range(args.runs):
                    if "b" in routes:
                        b.append(timed(device, args.warmup, args.iters) * 1e6)
                    if "a" in routes:
                        a.append(timed(baseline, 1, max(3, args.iters // 3)) * 1e6)
                    if "c" in routes:
                        c.append(timed(floor, args.warmup, args.iters) * 1e6)

                def col(x):
                    return {"median_us": round(statistics.median(x), 1), "min_us": round(min(x), 1),
                            "max_us": round(max(x), 1)} if x else None
                line = {"columns": shape, "elements": n, "row_len": per, "rows": rows, "bytes": length,
                        "a_host_roundtrip": col(a), "b_device_print_records": col(b), "c_printers_per_column": col(c)}
                if a and b:
                    line["b_beats_a_every_run"] = all(y < x for x, y in zip(a, b))
                    line["a_over_b"] = round(statistics.median(a) / statistics.median(b), 2)
                if b and c:
                    line["b_over_c"] = round(statistics.median(b) / statistics.median(c), 2)
                print(json.dumps(line), flush=True)
    print(json.dumps({"json_stats": native.gpu.json_stats()}))


if __name__ == "__main__":
    main()
