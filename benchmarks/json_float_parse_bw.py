"""What a float / double array costs to parse from JSON text, four ways:

  a  element-wise  json::Parse with packed numbers switched off
                   (native.json_parse_check(text, False)): std::from_chars
                   and a json::Value per element, the route the reader took
                   for every array with a float in it before packed numbers
  b  host packed   json::Parse (native.json_parse_check(text, True)): one
                   pass with base/decimal_to_double.h into 8 bytes and a
                   class byte per element
  c  device, host text   json::ParseWithIndex over a structural index made
                   beforehand (native.gpu.json_parse_with_index), the GPU
                   JSON path enabled and -gpu_json2pb_float_min_elems 1: the
                   integer offload is tried first and declines (a launch
                   and a wait), then gpu::ParseNumbersOnDevice (text and
                   separators staged in pinned memory, one launch sequence,
                   one wait, payload and classes copied out)
  d  device, HBM -> HBM  native.gpu.device_json_parse_numbers on text and
                   separators in device memory into a device array
  e  the op        ops.json_parse_floats on the same text: d and the
                   separators found with torch ops on the device

over "[v,v,...]" of standard-normal float32 / float64 values printed by
native.json_format_floats. a to c build and drop the DOM inside the timed
call. Every path is timed on the host around its blocking call, --warmup
untimed and --iters timed calls, the median reported; the whole sweep repeats
--runs times so that a crossover can be required of every run. Prints one
JSON line per kind, size and run, then the smallest size at which c beat b
in every run.

  python benchmarks/json_float_parse_bw.py [--sizes-ki 4,16,64,256,1024] [--runs 3]
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
PARSE_FLOAT64, PARSE_FLOAT32 = 1, 2


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
    args = ap.parse_args()
    from brpc_amd import native, ops
    assert torch.cuda.is_available() and native.gpu.device_count() > 0, "this benchmark needs the GPU"
    dev = torch.device("cuda", 0)
    sizes = [int(float(x) * 1024) for x in args.sizes_ki.split(",")]
    wins = {FLOAT: {n: 0 for n in sizes}, DOUBLE: {n: 0 for n in sizes}}
    flag_before = native.get_flag("gpu_json2pb_float_min_elems")
    for run in range(args.runs):
        for kind, dtype in ((FLOAT, np.float32), (DOUBLE, np.float64)):
            for n in sizes:
                vals = np.random.default_rng(n + kind).standard_normal(n).astype(dtype)
                text = b"[" + native.json_format_floats(vals.tobytes(), kind) + b"]"
                index = np.array(native.gpu.json_index_bytes(text, 0), dtype=np.uint32).tobytes()
                assert len(index) == 4 * (n + 1)  # the brackets and the commas
                want_payload, want_classes = native.json_parse_numbers(text)
                assert np.frombuffer(want_payload, dtype=np.float64).astype(dtype).tobytes() == vals.tobytes()
                dtext = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(dev)
                dseps = torch.from_numpy(np.frombuffer(index, dtype=np.int32).copy()).to(dev)
                out = torch.zeros(n, dtype=torch.float32 if kind == FLOAT else torch.float64, device=dev)
                mode = PARSE_FLOAT32 if kind == FLOAT else PARSE_FLOAT64
                torch.cuda.synchronize()

                def hbm():
                    return native.gpu.device_json_parse_numbers([dtext.data_ptr()], [dseps.data_ptr()], [n], [mode],
                                                                [out.data_ptr()], [0], [0], [0], 0)

                # every path parses the same values
                assert native.gpu.json_parse_numbers(text, 0)[:2] == (want_payload, want_classes)
                assert hbm() == [(0, 0xFFFFFFFF, 0)] and out.cpu().numpy().tobytes() == vals.tobytes()
                assert ops.json_parse_floats(dtext, dtype=out.dtype).cpu().numpy().tobytes() == vals.tobytes()
                assert native.json_parse_check(text, False) == (True, "") and native.json_parse_check(text, True) == (True, "")
                t_d = timed(hbm, args.warmup, args.iters)
                t_e = timed(lambda: ops.json_parse_floats(dtext, dtype=out.dtype), args.warmup, args.iters)
                native.set_flag("gpu_json2pb_float_min_elems", "1")
                native.gpu.enable_json_index(0, 65536)
                try:
                    s0 = native.gpu.json_stats()
                    assert native.gpu.json_parse_with_index(text, index) == (True, "")
                    s1 = native.gpu.json_stats()
                    assert s1["number_arrays"] - s0["number_arrays"] == 1 and s1["number_elems"] - s0["number_elems"] == n
                    t_c = timed(lambda: native.gpu.json_parse_with_index(text, index), args.warmup, args.iters)
                finally:
                    native.gpu.disable_json_index()
                    native.set_flag("gpu_json2pb_float_min_elems", str(flag_before))
                t_b = timed(lambda: native.json_parse_check(text, True), args.warmup, args.iters)
                t_a = timed(lambda: native.json_parse_check(text, False), 1, max(3, args.iters // 3))
                wins[kind][n] += t_c < t_b
                print(json.dumps({
                    "run": run, "kind": "float32" if kind == FLOAT else "float64", "elements": n,
                    "text_bytes": len(text),
                    "a_elementwise_us": round(t_a * 1e6, 1), "b_host_packed_us": round(t_b * 1e6, 1),
                    "c_device_from_host_us": round(t_c * 1e6, 1),
                    "d_hbm_to_hbm_us": round(t_d * 1e6, 1), "e_op_us": round(t_e * 1e6, 1),
                    "a_over_b": round(t_a / t_b, 1), "b_over_c": round(t_b / t_c, 2),
                    "d_text_gb_per_s": round(len(text) / t_d / 1e9, 2)}), flush=True)
    crossover = {}
    for kind, name in ((FLOAT, "float32"), (DOUBLE, "float64")):
        ok = [n for n in sizes if wins[kind][n] == args.runs]
        crossover[name] = min(ok) if ok else None
    print(json.dumps({"smallest_size_where_c_beats_b_in_every_run": crossover, "runs": args.runs,
                      "json_stats": native.gpu.json_stats()}))


if __name__ == "__main__":
    main()
