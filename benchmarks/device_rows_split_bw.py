"""A message of rows split where it lives (HBM -> HBM) into the flat array and
the row ends: gpu::DeviceSplitRows (native.gpu.device_split_rows), against
  (a)  what a handler had before it: a D2H copy of the message, the dynamic
       host parser on a .proto parsed at run time (native.pb_dynamic_parse:
       parse only; copying the parsed rows into a flat array would come on
       top, so this column is a lower bound), H2D copies of values and row_ends;
  (a') the same with the host twin (native.pb_split_rows) in the parser's place;
  (c)  the yardstick of the inverse: native.gpu.device_build_rows on the same
       data (the way the message was made).
Shapes: 4 Ki .. 1 Mi elements (--elems takes more) as rows of 1, 32 and 1024
elements and as one single row; uint32 ids below 2^14 (2-byte varints, kind 1)
and float32 (kind 8), each row a sub-message with the packed field 2. Every
call is timed on the host around the blocking call, warm-up calls first, the
median of --iters calls reported; the whole table is taken --runs times and
each figure printed with the range of the runs' medians. One JSON line per
shape.

  python benchmarks/device_rows_split_bw.py [--elems 4096,...] [--iters 20] [--runs 3]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

PROTO = ('syntax = "proto2";\nmessage Row { repeated %s v = 2 [packed = true]; }\n'
         'message Batch { repeated Row rows = 4; }\n')


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
    ap.add_argument("--row-lens", default="1,32,1024,0", help="elements per row; 0: one single row")
    ap.add_argument("--kinds", default="ids,float32")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--skip", type=int, default=0, help="-device_split_skip for this run (0: the default)")
    args = ap.parse_args()
    from brpc_amd import native
    if args.skip:
        native.set_flag("device_split_skip", str(args.skip))
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is no CPU figure"
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    tmp = tempfile.mkdtemp()
    for kind_name in args.kinds.split(","):
        kind = 1 if kind_name == "ids" else 8
        proto = "rows_%s.proto" % kind_name
        with open(os.path.join(tmp, proto), "w") as f:
            f.write(PROTO % ("uint32" if kind == 1 else "float"))
        for n in [int(x) for x in args.elems.split(",")]:
            vals = rng.integers(1 << 7, 1 << 14, n).astype(np.uint32) if kind == 1 else \
                rng.standard_normal(n).astype(np.float32)
            src = torch.from_numpy(vals.view(np.int32).copy()).to(dev)
            for row_len in [int(x) for x in args.row_lens.split(",")]:
                per = row_len or n
                ends_np = np.arange(per, n + 1, per, dtype=np.uint32)
                if ends_np.size == 0 or ends_np[-1] != n:
                    ends_np = np.append(ends_np, np.uint32(n))
                ends = torch.from_numpy(ends_np.view(np.int32).copy()).to(dev)
                rows = int(ends_np.size)
                cap = native.gpu.device_rows_worst_case(4, 2, kind, n, rows)
                msg = torch.empty(cap, dtype=torch.uint8, device=dev)
                build_job = [(4, 2, kind, src.data_ptr(), n, ends.data_ptr(), rows, msg.data_ptr(), cap)]
                torch.cuda.synchronize()  # the uploads run on torch's stream, the codecs on theirs
                (length, err, _), = native.gpu.device_build_rows(build_job, 0)
                assert err == 0, err
                if length > native.gpu.device_split_max_bytes():
                    continue
                # the receiver sizes its outputs by the message alone
                out_vals = torch.empty(length // (4 if kind == 8 else 1), dtype=torch.int32, device=dev)
                out_ends = torch.empty(length // 2, dtype=torch.int32, device=dev)
                split_job = [(4, 2, kind, msg.data_ptr(), length, out_vals.data_ptr(), out_vals.numel(),
                              out_ends.data_ptr(), out_ends.numel())]
                host_vals, host_ends = vals.view(np.int32), ends_np.view(np.int32)
                kept = []

                def split():
                    return native.gpu.device_split_rows(split_job, 0)

                def roundtrip(parse):
                    wire = msg[:length].cpu().numpy().tobytes()
                    got = parse(wire)
                    kept[:] = [torch.from_numpy(got[0]).to(dev), torch.from_numpy(got[1]).to(dev)]
                    torch.cuda.synchronize()

                def dynamic(wire):
                    assert native.pb_dynamic_parse(tmp, proto, "Batch", wire)
                    return host_vals, host_ends

                def twin(wire):
                    r = native.pb_split_rows(4, 2, kind, wire)
                    return np.frombuffer(r[5], dtype=np.int32), np.asarray(r[6], dtype=np.int32)

                def build():
                    return native.gpu.device_build_rows(build_job, 0)

                (count, nrows, _, err, _), = split()
                assert (count, nrows, err) == (n, rows, 0), (count, nrows, err)
                assert torch.equal(out_vals[:n], src) and torch.equal(out_ends[:rows], ends)
                roundtrip(twin)
                assert torch.equal(kept[0], src) and torch.equal(kept[1], ends)
                a, a2, b, c = [], [], [], []
                for _ in range(args.runs):
                    b.append(timed(split, args.warmup, args.iters) * 1e6)
                    a.append(timed(lambda: roundtrip(dynamic), 1, max(3, args.iters // 4)) * 1e6)
                    a2.append(timed(lambda: roundtrip(twin), 1, max(3, args.iters // 4)) * 1e6)
                    c.append(timed(build, args.warmup, args.iters) * 1e6)

                def col(x):
                    return {"median_us": round(statistics.median(x), 1), "min_us": round(min(x), 1),
                            "max_us": round(max(x), 1)}
                print(json.dumps({"kind": kind_name, "elements": n, "row_len": per, "rows": rows, "bytes": length,
                                  "a_host_dynamic_parser": col(a), "a2_host_twin": col(a2), "b_device_split": col(b),
                                  "c_device_build": col(c),
                                  "b_beats_a_every_run": all(y < x for x, y in zip(a, b)),
                                  "a_over_b": round(statistics.median(a) / statistics.median(b), 2),
                                  "b_over_c": round(statistics.median(b) / statistics.median(c), 2)}), flush=True)
    print(json.dumps({"device_codec_stats": native.gpu.device_codec_stats()}))


if __name__ == "__main__":
    main()
