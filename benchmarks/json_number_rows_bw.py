"""What a number array or a ragged batch of number rows that sits in HBM costs
to turn into JSON text in HBM, four ways:

  a  through the host      D2H of the values and the row ends, the host twin
                           native.json_format_number_rows
                           (json::FormatNumberRows), H2D of the text: what a
                           handler does without a device printer
  b  device, rows          native.gpu.device_json_print_numbers
                           (gpu::DevicePrintNumbers), one job: [[v,..],..] for
                           the row shapes, [v,..] for the flat one
  c  the floor             the same elements as one flat v,v,...,v: for floats
                           native.gpu.device_json_print_floats
                           (gpu::DevicePrintFloatArrays), for integers the new
                           entry without brackets. b / c is what rows cost
  d  device, job per row   float rows only: device_json_print_floats with one
                           job per row, each into its own slot of the output,
                           which is the device route there was for rows (it
                           still leaves the brackets and commas to the caller)

for int32 ids uniform in [0, 128000), int64 of mixed widths and float32
standard normals; 4 Ki, 64 Ki and 1 Mi elements, each flat and in rows of 32
and of 1024. Every path is timed on the host around its blocking call (the
device paths end in a wait for the stream), --warmup untimed and --iters timed
calls, the median taken; the whole sweep repeats --runs times. Prints one JSON
line per input, size, shape and run, then per input, size and shape the
median over the runs.

  python benchmarks/json_number_rows_bw.py [--sizes-ki 4,64,1024] [--runs 3]
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

INT32, INT64, FLOAT = 0, 3, 8
PATHS = ("a_through_host_us", "b_device_rows_us", "c_flat_floor_us", "d_job_per_row_us")


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


def make_values(name, n):
    rng = np.random.default_rng(n)
    if name == "int32_ids":
        return INT32, rng.integers(0, 128000, n).astype(np.int32)
    if name == "int64_mixed":
        v = rng.integers(0, 1 << 62, n, dtype=np.int64) >> rng.integers(0, 62, n)
        return INT64, np.where(rng.integers(0, 2, n) == 1, v, -v).astype(np.int64)
    return FLOAT, rng.standard_normal(n).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes-ki", default="4,64,1024")
    ap.add_argument("--rows-of", default="0,32,1024", help="row lengths; 0 is the flat array")
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    from brpc_amd import native
    assert torch.cuda.is_available() and native.gpu.device_count() > 0, "this benchmark needs the GPU"
    dev = torch.device("cuda", 0)
    sizes = [int(float(x) * 1024) for x in args.sizes_ki.split(",")]
    shapes = [int(x) for x in args.rows_of.split(",")]
    seen = {}
    for run in range(args.runs):
        for name in ("int32_ids", "int64_mixed", "float32_normal"):
            for n in sizes:
                kind, vals = make_values(name, n)
                src = torch.from_numpy(vals).to(dev)
                for row in shapes:
                    rows = n // row if row else 0
                    ends_host = np.arange(1, rows + 1, dtype=np.uint32) * np.uint32(row)
                    ends = torch.from_numpy(ends_host.view(np.int32).copy()).to(dev) if rows else None
                    cap = native.gpu.json_number_print_worst_case(kind, n, rows)
                    dst = torch.empty(cap, dtype=torch.uint8, device=dev)
                    err, _, want = native.json_format_number_rows(vals.tobytes(), n, kind,
                                                                  ends_host.tobytes() if rows else None, True)
                    assert err == 0
                    torch.cuda.synchronize()

                    def through_host():
                        image = src.cpu().numpy().tobytes()
                        table = ends.cpu().numpy().tobytes() if rows else None
                        text = native.json_format_number_rows(image, n, kind, table, True)[2]
                        out = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)
                        torch.cuda.synchronize()
                        return out

                    def device_rows():
                        return native.gpu.device_json_print_numbers(
                            [src.data_ptr()], [n], [kind], [ends.data_ptr() if rows else 0], [rows], [True],
                            [dst.data_ptr()], [cap], 0)

                    def floor():
                        if kind == FLOAT:
                            return native.gpu.device_json_print_floats([src.data_ptr()], [n], [kind], [dst.data_ptr()],
                                                                       [cap], 0)
                        return native.gpu.device_json_print_numbers([src.data_ptr()], [n], [kind], [0], [0], [False],
                                                                    [dst.data_ptr()], [cap], 0)

                    # every path prints the same bytes
                    assert bytes(through_host().cpu().numpy()) == want
                    (length, _, err), = device_rows()
                    assert err == 0 and bytes(dst[:length].cpu().numpy()) == want
                    line = {"run": run, "input": name, "elements": n, "rows_of": row, "text_bytes": len(want)}
                    line[PATHS[0]] = timed(through_host, args.warmup, args.iters) * 1e6
                    line[PATHS[1]] = timed(device_rows, args.warmup, args.iters) * 1e6
                    line[PATHS[2]] = timed(floor, args.warmup, args.iters) * 1e6
                    if kind == FLOAT and rows:
                        slot = native.gpu.json_float_worst_case(row)
                        slots = torch.empty(rows * slot, dtype=torch.uint8, device=dev)
                        srcs = [src.data_ptr() + 4 * row * r for r in range(rows)]
                        dsts = [slots.data_ptr() + slot * r for r in range(rows)]
                        counts, kinds, caps = [row] * rows, [kind] * rows, [slot] * rows

                        def job_per_row():
                            return native.gpu.device_json_print_floats(srcs, counts, kinds, dsts, caps, 0)

                        assert all(e == 0 for _, e in job_per_row())
                        line[PATHS[3]] = timed(job_per_row, args.warmup, args.iters) * 1e6
                    line["b_over_c"] = line[PATHS[1]] / line[PATHS[2]]
                    line["a_over_b"] = line[PATHS[0]] / line[PATHS[1]]
                    seen.setdefault((name, n, row), []).append(line)
                    print(json.dumps({k: round(v, 2) if isinstance(v, float) else v for k, v in line.items()}),
                          flush=True)
    print("median over %d runs (us per blocking call):" % args.runs)
    print("| input | elements | rows of | text bytes | a host | b rows | c flat | d job/row | b/c | a/b |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for (name, n, row), lines in seen.items():
        med = {k: statistics.median(x[k] for x in lines) for k in PATHS + ("b_over_c", "a_over_b") if k in lines[0]}
        d = "%.0f" % med[PATHS[3]] if PATHS[3] in med else "-"
        print("| %s | %d | %s | %d | %.0f | %.0f | %.0f | %s | %.2f | %.2f |"
              % (name, n, row or "flat", lines[0]["text_bytes"], med[PATHS[0]], med[PATHS[1]], med[PATHS[2]], d,
                 med["b_over_c"], med["a_over_b"]))


if __name__ == "__main__":
    main()
