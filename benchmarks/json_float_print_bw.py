"""What a float / double array costs to print as JSON text, four ways:

  a  element-wise  json::AppendShortestDouble per element (snprintf + strtod
                   rounds), the printer pb2json used for these fields before
                   the host twin: native.json_shortest_double per element,
                   timed on a sample of at most --oracle-elems elements and
                   scaled to the array (the Python call overhead, measured on
                   a no-op binding call, is subtracted)
  b  host twin     native.json_format_floats (json2pb::FormatFloatArray)
  c  device, host values   native.gpu.json_print_floats
                   (gpu::PrintFloatsOnDevice: pinned stage, three launches,
                   text written to pinned memory, one wait; staging included)
  d  device, HBM -> HBM    native.gpu.device_json_print_floats on a device
                   array into a device buffer

for float32 and float64 arrays of normally distributed values. Every path is
timed on the host around its blocking call (the device paths end in a wait
for the stream), --warmup untimed and --iters timed calls, the median
reported; the whole sweep repeats --runs times so that a crossover can be
required of every run. Prints one JSON line per kind, size and run, then the
smallest size at which c beat b in every run.

  python benchmarks/json_float_print_bw.py [--sizes-ki 4,16,64,256,1024] [--runs 3]
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

FLOAT, DOUBLE = 8, 9


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
    ap.add_argument("--sizes-ki", default="4,16,64,256,1024")
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--oracle-elems", type=int, default=16384)
    args = ap.parse_args()
    from brpc_amd import native
    assert torch.cuda.is_available() and native.gpu.device_count() > 0, "this benchmark needs the GPU"
    dev = torch.device("cuda", 0)
    sizes = [int(float(x) * 1024) for x in args.sizes_ki.split(",")]
    wins = {FLOAT: {n: 0 for n in sizes}, DOUBLE: {n: 0 for n in sizes}}
    for run in range(args.runs):
        for kind, dtype in ((FLOAT, np.float32), (DOUBLE, np.float64)):
            for n in sizes:
                vals = np.random.default_rng(n + kind).standard_normal(n).astype(dtype)
                raw = vals.tobytes()
                want = native.json_format_floats(raw, kind)
                src = torch.from_numpy(vals).to(dev)
                cap = native.gpu.json_float_worst_case(n)
                dst = torch.empty(cap, dtype=torch.uint8, device=dev)
                torch.cuda.synchronize()

                def hbm():
                    return native.gpu.device_json_print_floats([src.data_ptr()], [n], [kind], [dst.data_ptr()], [cap], 0)

                # every path prints the same bytes
                assert native.gpu.json_print_floats(raw, n, kind, 0) == want
                (length, err), = hbm()
                assert err == 0 and bytes(dst[:length].cpu().numpy()) == want
                t_d = timed(hbm, args.warmup, args.iters)
                t_c = timed(lambda: native.gpu.json_print_floats(raw, n, kind, 0), args.warmup, args.iters)
                t_b = timed(lambda: native.json_format_floats(raw, kind), args.warmup, args.iters)
                sample = [float(x) for x in vals[:min(n, args.oracle_elems)]]

                def oracle():
                    f = native.json_shortest_double
                    for x in sample:
                        f(x)

                def call_overhead():
                    f = native.get_concurrency
                    for _ in sample:
                        f()

                t_a = max(timed(oracle, 1, 3) - timed(call_overhead, 1, 3), 0.0) * n / len(sample)
                wins[kind][n] += t_c < t_b
                print(json.dumps({
                    "run": run, "kind": "float32" if kind == FLOAT else "float64", "elements": n,
                    "text_bytes": len(want),
                    "a_elementwise_us": round(t_a * 1e6, 1), "b_host_twin_us": round(t_b * 1e6, 1),
                    "c_device_from_host_us": round(t_c * 1e6, 1),
                    "d_hbm_to_hbm_us": round(t_d * 1e6, 1),
                    "a_over_b": round(t_a / t_b, 1), "b_over_c": round(t_b / t_c, 2),
                    "d_text_gb_per_s": round(len(want) / t_d / 1e9, 2)}), flush=True)
    crossover = {}
    for kind, name in ((FLOAT, "float32"), (DOUBLE, "float64")):
        ok = [n for n in sizes if wins[kind][n] == args.runs]
        crossover[name] = min(ok) if ok else None
    print(json.dumps({"smallest_size_where_c_beats_b_in_every_run": crossover, "runs": args.runs,
                      "json_stats": native.gpu.json_stats()}))


if __name__ == "__main__":
    main()
