"""What a float / double array costs to parse from JSON text:

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
  e  the op        ops.json_parse_floats on the same text: one call of f,
                   the output sized for the worst case
  f  device, HBM text alone  native.gpu.device_json_parse_text: the same
                   text with no separator table (the device counts, ranks
                   and converts), into a device array of n elements
  g  the op as it was  d behind separators found with torch ops on the
                   device (nonzero, cat, where and two reads of single
                   bytes): what ops.json_parse_floats did before f existed
  h  rows          the same values as "[[v x 1024],[...],...]": f on that
                   text with a row_ends buffer (h_rows_entry_us) and
                   ops.json_parse_float_rows (h_rows_op_us)

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


def op_with_torch_separators(native, t, dtype, mode):
    """Column g: the separator pass ops.json_parse_floats ran before the
    device found the elements itself (bracketed text, no redo elements)."""
    dev, n = t.device, t.numel()
    assert int(t[0]) == 0x5B and int(t[-1]) == 0x5D
    commas = torch.nonzero(t == 0x2C).view(-1)
    seps64 = torch.cat([torch.tensor([0], dtype=torch.int64, device=dev), commas,
                        torch.tensor([n - 1], dtype=torch.int64, device=dev)])
    seps = torch.where(seps64 >= 1 << 31, seps64 - (1 << 32), seps64).to(torch.int32)
    count = seps.numel() - 1
    out = torch.zeros(count, dtype=dtype, device=dev)
    redo = torch.zeros(64, dtype=torch.int32, device=dev)
    torch.cuda.current_stream(dev).synchronize()
    (err, _, n_redo), = native.gpu.device_json_parse_numbers([t.data_ptr()], [seps.data_ptr()], [count], [mode],
                                                             [out.data_ptr()], [0], [redo.data_ptr()], [64], 0)
    assert err == 0 and n_redo == 0
    return out


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

                def text_entry():
                    return native.gpu.device_json_parse_text([dtext.data_ptr()], [len(text)], [mode], [out.data_ptr()],
                                                             [0], [n], [0], [0], [0], [0], 0)

                # the same values in rows of 1024 (one short row when n is no multiple)
                row_texts = [native.json_format_floats(vals[i:i + 1024].tobytes(), kind) for i in range(0, n, 1024)]
                nested = b"[[" + b"],[".join(row_texts) + b"]]"
                dnested = torch.from_numpy(np.frombuffer(nested, dtype=np.uint8).copy()).to(dev)
                row_ends = torch.zeros(len(row_texts), dtype=torch.int32, device=dev)

                def rows_entry():
                    return native.gpu.device_json_parse_text([dnested.data_ptr()], [len(nested)], [mode], [out.data_ptr()],
                                                             [0], [n], [row_ends.data_ptr()], [len(row_texts)], [0], [0], 0)

                # every path parses the same values
                out.zero_()
                assert text_entry() == [(0, 1, n, 0, 0, 0xFFFFFFFF)] and out.cpu().numpy().tobytes() == vals.tobytes()
                out.zero_()
                assert rows_entry() == [(0, 2, n, len(row_texts), 0, 0xFFFFFFFF)]
                assert out.cpu().numpy().tobytes() == vals.tobytes()
                assert row_ends.tolist() == [min(i + 1024, n) for i in range(0, n, 1024)]
                assert ops.json_parse_float_rows(dnested, dtype=out.dtype, ragged=True)[0].cpu().numpy().tobytes() == vals.tobytes()
                assert op_with_torch_separators(native, dtext, out.dtype, mode).cpu().numpy().tobytes() == vals.tobytes()
                out.zero_()
                assert native.gpu.json_parse_numbers(text, 0)[:2] == (want_payload, want_classes)
                assert hbm() == [(0, 0xFFFFFFFF, 0)] and out.cpu().numpy().tobytes() == vals.tobytes()
                assert ops.json_parse_floats(dtext, dtype=out.dtype).cpu().numpy().tobytes() == vals.tobytes()
                assert native.json_parse_check(text, False) == (True, "") and native.json_parse_check(text, True) == (True, "")
                t_d = timed(hbm, args.warmup, args.iters)
                t_e = timed(lambda: ops.json_parse_floats(dtext, dtype=out.dtype), args.warmup, args.iters)
                t_f = timed(text_entry, args.warmup, args.iters)
                t_g = timed(lambda: op_with_torch_separators(native, dtext, out.dtype, mode), args.warmup, args.iters)
                t_hf = timed(rows_entry, args.warmup, args.iters)
                t_ho = timed(lambda: ops.json_parse_float_rows(dnested, dtype=out.dtype, ragged=n % 1024 != 0),
                             args.warmup, args.iters)
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
                    "f_text_entry_us": round(t_f * 1e6, 1), "g_op_torch_separators_us": round(t_g * 1e6, 1),
                    "h_rows_entry_us": round(t_hf * 1e6, 1), "h_rows_op_us": round(t_ho * 1e6, 1),
                    "a_over_b": round(t_a / t_b, 1), "b_over_c": round(t_b / t_c, 2), "g_over_e": round(t_g / t_e, 2),
                    "d_text_gb_per_s": round(len(text) / t_d / 1e9, 2)}), flush=True)
    crossover = {}
    for kind, name in ((FLOAT, "float32"), (DOUBLE, "float64")):
        ok = [n for n in sizes if wins[kind][n] == args.runs]
        crossover[name] = min(ok) if ok else None
    print(json.dumps({"smallest_size_where_c_beats_b_in_every_run": crossover, "runs": args.runs,
                      "json_stats": native.gpu.json_stats()}))


if __name__ == "__main__":
    main()
