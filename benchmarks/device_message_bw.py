"""One protobuf message with a large packed field, built where the values
already live (HBM -> HBM): gpu::DeviceBuildMessages (native.gpu.device_build_message)
against the path a handler had before it on the same array:
  D2H copy of the values, native.gpu.pb_run_encode on the host copy (the
  host sizes every element, the device encodes from the host's pages), and
  an H2D copy of the encoded bytes.
Both are timed on the host around the blocking calls, 3 warm-up and 20 timed
calls each, the median reported. Sizes are the encoded run's bytes. Prints
one JSON line per shape and size.

  python benchmarks/device_message_bw.py [--sizes-mb 1,16,64] [--iters 20]
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
    ap.add_argument("--sizes-mb", default="1,16,64")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="ids,u64", help="ids: int32 ids < 2^14 (2-byte varints); u64: full-width")
    args = ap.parse_args()
    from brpc_amd import native
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    for shape in args.shapes.split(","):
        kind, per = (0, 2) if shape == "ids" else (4, 10)
        for mb in [float(x) for x in args.sizes_mb.split(",")]:
            n = int(mb * (1 << 20)) // per
            vals = rng.integers(1 << 7, 1 << 14, n).astype(np.int32) if shape == "ids" else \
                rng.integers(1 << 63, (1 << 64) - 1, n, dtype=np.uint64)
            src = torch.from_numpy(vals.view(np.int32 if kind == 0 else np.int64)).to(dev)
            rows = [(8, kind, src.data_ptr(), n)]
            cap = native.gpu.device_message_worst_case(rows)
            dst = torch.empty(cap, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()  # the upload runs on torch's stream, the builder on ours

            def build():
                return native.gpu.device_build_message(rows, dst.data_ptr(), cap, 0)

            uploaded = []

            def baseline():
                host = src.cpu().numpy()
                wire = native.gpu.pb_run_encode(host.tobytes(), n, kind)
                uploaded[:] = [torch.frombuffer(bytearray(wire), dtype=torch.uint8).to(dev)]
                torch.cuda.synchronize()

            length, err, [(off, plen)] = build()
            assert err == 0 and plen == n * per, (length, err, plen)
            baseline()
            # the two paths make the same run
            assert torch.equal(dst[off:off + plen], uploaded[0])
            t_build = timed(build, args.warmup, args.iters)
            t_base = timed(baseline, args.warmup, args.iters)
            print(json.dumps({"shape": shape, "run_bytes": plen, "elements": n,
                              "build_us": round(t_build * 1e6, 1), "baseline_us": round(t_base * 1e6, 1),
                              "baseline_over_build": round(t_base / t_build, 2),
                              "build_out_gb_per_s": round(plen / t_build / 1e9, 2)}), flush=True)
    print(json.dumps({"device_codec_stats": native.gpu.device_codec_stats(),
                      "codec_batch_stats": native.gpu.codec_batch_stats()}))


if __name__ == "__main__":
    main()
