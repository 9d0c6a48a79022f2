"""A ragged batch serialized where it lives (HBM -> HBM) as the rows of one
repeated field: gpu::DeviceBuildRows (native.gpu.device_build_rows), against
  (a) what a handler had before it: D2H copies of the values and of row_ends,
      the host twin (native.pb_serialize_rows), an H2D copy of the bytes;
  (c) the floor: native.gpu.device_build_message on the same values as ONE
      flat packed (ids) or bytes (floats) field, no rows at all.
Shapes: 4 Ki .. 1 Mi elements as rows of 1, 32 and 1024 elements and as one
single row; uint32 ids below 2^14 (2-byte varints, kind 1) and float32 (kind
8), each row a sub-message with the packed field 2. Every call is timed on
the host around the blocking call (the builders wait for their stream, the
baseline ends in a device synchronize), warm-up calls first, the median of
--iters calls reported; the whole table is taken --runs times and each
figure printed with the range of the runs' medians. One JSON line per shape.

  python benchmarks/device_rows_bw.py [--elems 4096,...] [--iters 20] [--runs 3]
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
    ap.add_argument("--elems", default="4096,16384,65536,262144,1048576")
    ap.add_argument("--row-lens", default="1,32,1024,0", help="elements per row; 0: one single row")
    ap.add_argument("--kinds", default="ids,float32")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    from brpc_amd import native
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is no CPU figure"
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    for kind_name in args.kinds.split(","):
        kind, flat_kind = (1, 1) if kind_name == "ids" else (8, 7)
        for n in [int(x) for x in args.elems.split(",")]:
            vals = rng.integers(1 << 7, 1 << 14, n).astype(np.uint32) if kind == 1 else \
                rng.standard_normal(n).astype(np.float32)
            src = torch.from_numpy(vals.view(np.int32).copy()).to(dev)
            flat = [(8, flat_kind, src.data_ptr(), n * 4 if flat_kind == 7 else n)]
            flat_cap = native.gpu.device_message_worst_case(flat)
            flat_dst = torch.empty(flat_cap, dtype=torch.uint8, device=dev)
            for row_len in [int(x) for x in args.row_lens.split(",")]:
                per = row_len or n
                ends_np = np.arange(per, n + 1, per, dtype=np.uint32)
                if ends_np.size == 0 or ends_np[-1] != n:
                    ends_np = np.append(ends_np, np.uint32(n))
                ends = torch.from_numpy(ends_np.view(np.int32).copy()).to(dev)
                rows = int(ends_np.size)
                cap = native.gpu.device_rows_worst_case(4, 2, kind, n, rows)
                dst = torch.empty(cap, dtype=torch.uint8, device=dev)
                job = [(4, 2, kind, src.data_ptr(), n, ends.data_ptr(), rows, dst.data_ptr(), cap)]
                torch.cuda.synchronize()  # the uploads run on torch's stream, the builders on theirs
                uploaded = []

                def build():
                    return native.gpu.device_build_rows(job, 0)

                def baseline():
                    host_vals = src.cpu().numpy()
                    host_ends = ends.cpu().numpy()
                    err, _, wire = native.pb_serialize_rows(4, 2, kind, host_vals.tobytes(), host_ends.tobytes())
                    uploaded[:] = [torch.frombuffer(bytearray(wire), dtype=torch.uint8).to(dev)]
                    torch.cuda.synchronize()

                def floor():
                    return native.gpu.device_build_message(flat, flat_dst.data_ptr(), flat_cap, 0)

                (length, err, _), = build()
                assert err == 0, err
                baseline()
                assert torch.equal(dst[:length], uploaded[0])  # the two paths make the same bytes
                assert floor()[1] == 0
                a, b, c = [], [], []
                for _ in range(args.runs):
                    b.append(timed(build, args.warmup, args.iters) * 1e6)
                    a.append(timed(baseline, args.warmup, args.iters) * 1e6)
                    c.append(timed(floor, args.warmup, args.iters) * 1e6)

                def col(x):
                    return {"median_us": round(statistics.median(x), 1), "min_us": round(min(x), 1),
                            "max_us": round(max(x), 1)}
                print(json.dumps({"kind": kind_name, "elements": n, "row_len": per, "rows": rows, "bytes": length,
                                  "a_host_roundtrip": col(a), "b_device_rows": col(b), "c_flat_field": col(c),
                                  "b_wins_every_run": all(y < x for x, y in zip(a, b)),
                                  "a_over_b": round(statistics.median(a) / statistics.median(b), 2),
                                  "b_over_c": round(statistics.median(b) / statistics.median(c), 2)}), flush=True)
    print(json.dumps({"device_codec_stats": native.gpu.device_codec_stats()}))


if __name__ == "__main__":
    main()
