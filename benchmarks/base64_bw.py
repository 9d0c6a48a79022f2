"""What base64 of a buffer costs, each way (encode: data -> text, decode:
text -> data), seven ways:

  a  byte-wise host   the coder base/util.cc had before base/base64.h (kept
                      in benchmarks/base64_bytewise.cc), timed inside C++
  b  host twin        base64_encode / base64_decode of base/util.cc, timed
                      the same way
  c  what a handler with the buffer in HBM had before: D2H into pinned
                      memory, the host twin between pinned buffers, H2D
  d  device, HBM -> HBM   native.gpu.device_base64_encode / _decode, dst
                      16-byte aligned
  e  the same with dst off by one byte
  f  host bytes through the device, for information: a copy into a pinned
                      tensor, H2D, ops.json.base64_encode / _decode, D2H
  g  a torch device copy that moves as many bytes as d does (it reads n
                      and writes 4n/3, or the reverse: a copy of 7n/6
                      bytes), the memory-bound yardstick

over random data of 4 KiB to 64 MiB. c to g are timed on the host around
the blocking call (g with a device synchronize), --warmup untimed and a few
timed calls, the median reported; GB/s is of data bytes. The sweep repeats
--runs times. Prints one JSON line per direction, size and run, then the
acceptance comparisons (b faster than a at every size, d faster than c from
64 KiB, both in every run; d against g). --cpu-only times a and b alone, on
a machine without a GPU.

  python benchmarks/base64_bw.py [--sizes-ki 4,64,1024,16384,65536] [--runs 3]
  python benchmarks/base64_bw.py --table profiles/base64.txt   # the README table

--only rows measures the rows form instead (gpu::DeviceBase64EncodeRows /
DeviceBase64DecodeRows: `repeated bytes` <-> a JSON array of base64 strings):
random bytes in rows of 1, 32 and 1024 bytes and in one row, at 4 KiB, 64 KiB,
1 MiB and 64 MiB, each way, four routes, the median microseconds of a blocking
call, three runs:

  a  what a handler had: D2H of bytes and row_ends into pinned memory, the
     host twin (json::EncodeBase64Rows / DecodeBase64Rows), H2D of the result
  b  the rows entry, HBM -> HBM
  c  the flat DeviceBase64Encode / Decode over the same bytes as one buffer
     (for decode: over the symbols alone, without quotes and commas): the floor
  d  encode only: one flat job per row in one call, with the host copy of
     row_ends it needs (D2H, timed) and without the quotes and commas: the
     device route there was. Left out above --max-flat-jobs rows.

  python benchmarks/base64_bw.py --only rows > profiles/base64_rows.txt
  python benchmarks/base64_bw.py --only rows --table profiles/base64_rows.txt
"""
import argparse
import base64
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def load_helper():
    """benchmarks/base64_bytewise.cc as build/lib/libbase64_bw.so (built
    with the project's host flags against libmrpc when missing or stale)."""
    src = os.path.join(ROOT, "benchmarks", "base64_bytewise.cc")
    so = os.path.join(ROOT, "build", "lib", "libbase64_bw.so")
    libdir = os.path.join(ROOT, "brpc_amd", "lib")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.run(["g++", "-std=c++17", "-O2", "-march=x86-64-v2", "-fPIC", "-shared",
                        "-I" + os.path.join(ROOT, "brpc_amd", "csrc"), src, "-o", so, "-L" + libdir, "-lmrpc",
                        "-Wl,-rpath," + libdir], check=True)
    lib = ctypes.CDLL(so)
    lib.base64_bw_time.restype = ctypes.c_double
    lib.base64_bw_time.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p,
                                   ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    lib.base64_bw_host.restype = ctypes.c_size_t
    lib.base64_bw_host.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
    return lib


def iters_for(n, iters):
    return iters if n <= (1 << 20) else max(3, iters // 3)


def host_pair(lib, decode, src, want, warmup, iters):
    """(median seconds of a, of b), each result checked against `want`."""
    out = ctypes.create_string_buffer(len(want) + 16)
    got = ctypes.c_size_t(0)
    med = []
    for which in (0, 1):
        ts = []
        for i in range(warmup + iters):
            t = lib.base64_bw_time(which, decode, src, len(src), out, len(out), ctypes.byref(got))
            assert t >= 0 and out.raw[:got.value] == want
            if i >= warmup:
                ts.append(t)
        med.append(statistics.median(ts))
    return med


def timed(call, sync, warmup, iters):
    for _ in range(warmup):
        call()
    out = []
    for _ in range(iters):
        sync()
        t0 = time.perf_counter()
        call()
        out.append(time.perf_counter() - t0)
    return statistics.median(out)


def table(path):
    """The README table from a profile: medians over the runs found there."""
    rows = {}
    for line in open(path):
        line = line.strip()
        if not line.startswith('{"run"'):
            continue
        r = json.loads(line)
        if "d_hbm_us" in r:
            rows.setdefault((r["direction"], r["data_bytes"]), []).append(r)
    print("| direction | data | a byte-wise host | b host twin | c D2H + b + H2D | d device | e device, dst + 1 | "
          "d GB/s | d / g |")
    print("|---|---|---|---|---|---|---|---|---|")
    for (direction, n), rs in sorted(rows.items(), key=lambda kv: (kv[0][0] != "encode", kv[0][1])):
        def med(k):
            return statistics.median(r[k] for r in rs)
        name = "%d KiB" % (n >> 10) if n < 1 << 20 else "%d MiB" % (n >> 20)
        print("| %s | %s | %.1f µs | %.1f µs | %.1f µs | %.1f µs | %.1f µs | %.1f | %.2f |" % (
            direction, name, med("a_bytewise_us"), med("b_twin_us"), med("c_d2h_twin_h2d_us"), med("d_hbm_us"),
            med("e_hbm_dst_plus_1_us"), med("d_data_gb_per_s"), med("d_over_g")))


def rows_table(path):
    """The README table of the rows form from a profile: medians over the runs, and the ranges."""
    rows = {}
    for line in open(path):
        line = line.strip()
        if not line.startswith('{"run"'):
            continue
        r = json.loads(line)
        if "b_rows_us" in r:
            rows.setdefault((r["direction"], r["data_bytes"], r["row_bytes"]), []).append(r)
    print("| direction | data | row | a D2H + twin + H2D | b rows entry | c flat floor | d job per row | a / b | b / c | "
          "b range |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for (direction, n, width), rs in sorted(rows.items(), key=lambda kv: (kv[0][0] != "encode", kv[0][1], kv[0][2] or 1 << 40)):
        def med(k):
            vals = [r[k] for r in rs if r.get(k) is not None]
            return statistics.median(vals) if vals else None
        name = "%d KiB" % (n >> 10) if n < 1 << 20 else "%d MiB" % (n >> 20)
        d = med("d_job_per_row_us")
        bs = [r["b_rows_us"] for r in rs]
        print("| %s | %s | %s | %.1f µs | %.1f µs | %.1f µs | %s | %.2f | %.2f | %.1f .. %.1f |" % (
            direction, name, "one row" if not width else "%d B" % width, med("a_d2h_twin_h2d_us"), med("b_rows_us"),
            med("c_flat_us"), "-" if d is None else "%.1f µs" % d, med("a_d2h_twin_h2d_us") / med("b_rows_us"),
            med("b_rows_us") / med("c_flat_us"), min(bs), max(bs)))


def rows_main(args):
    import torch
    from brpc_amd import native
    assert torch.cuda.is_available() and native.gpu.device_count() > 0, "this benchmark needs the GPU"
    dev = torch.device("cuda", 0)
    g = native.gpu
    sync = torch.cuda.synchronize
    sizes = [int(float(x) * 1024) for x in args.sizes_ki.split(",")]

    def pinned(nbytes):
        return torch.empty(max(nbytes, 1), dtype=torch.uint8).pin_memory()

    def device_bytes(b):
        return torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).to(dev)

    for run in range(args.runs):
        for n in sizes:
            for width in (1, 32, 1024, 0):
                iters = iters_for(n, args.iters)
                data = np.random.default_rng(n + run).integers(0, 256, n, dtype=np.uint8)
                ends = np.arange(width, n + 1, width, dtype=np.uint32) if width else np.array([n], dtype=np.uint32)
                rows = len(ends)
                cap = g.base64_rows_worst_case(n, rows, True)
                d_data, d_ends = torch.from_numpy(data).to(dev), torch.from_numpy(ends.view(np.int32)).to(dev)
                d_text = torch.zeros(cap + 16, dtype=torch.uint8, device=dev)
                p_data, p_ends, p_text = pinned(n), pinned(4 * rows), pinned(cap)

                def enc_before():  # a
                    p_data[:n].copy_(d_data)
                    p_ends[:4 * rows].copy_(d_ends.view(torch.uint8))
                    sync()
                    got, _ = native.base64_rows_twin(0, p_data.data_ptr(), n, p_text.data_ptr(), cap, p_ends.data_ptr(), rows)
                    d_text[:got].copy_(p_text[:got])
                    sync()
                    return got

                def enc_rows():  # b
                    return g.device_base64_encode_rows([d_data.data_ptr()], [n], [d_ends.data_ptr()], [rows], True,
                                                       [d_text.data_ptr()], [cap], 0)[0]

                def enc_flat():  # c
                    return g.device_base64_encode([d_data.data_ptr()], [n], [d_text.data_ptr()], [cap], 0)[0]

                def enc_per_row():  # d
                    p_ends[:4 * rows].copy_(d_ends.view(torch.uint8))
                    sync()
                    e = p_ends[:4 * rows].numpy().view(np.uint32).astype(np.int64)
                    starts = np.concatenate(([0], e[:-1]))
                    lens = e - starts
                    outs = (starts + 2) // 3 * 4 + 3 * np.arange(rows)  # room for what the rows form would take
                    return g.device_base64_encode((d_data.data_ptr() + starts).tolist(), lens.tolist(),
                                                  (d_text.data_ptr() + outs).tolist(), ((lens + 2) // 3 * 4).tolist(), 0)

                want = native.base64_encode_rows(data.tobytes(), ends.tobytes(), True)
                tlen = len(want)
                assert enc_before() == tlen and d_text[:tlen].cpu().numpy().tobytes() == want
                d_text.zero_()
                assert tuple(enc_rows()[:2]) == (tlen, 0) and d_text[:tlen].cpu().numpy().tobytes() == want
                row = {"run": run, "direction": "encode", "data_bytes": n, "row_bytes": width, "rows": rows,
                       "text_bytes": tlen,
                       "a_d2h_twin_h2d_us": round(timed(enc_before, sync, args.warmup, iters) * 1e6, 1),
                       "b_rows_us": round(timed(enc_rows, sync, args.warmup, iters) * 1e6, 1),
                       "c_flat_us": round(timed(enc_flat, sync, args.warmup, iters) * 1e6, 1),
                       "d_job_per_row_us": None}
                if rows <= args.max_flat_jobs:
                    assert all(r[1] == 0 for r in enc_per_row())
                    row["d_job_per_row_us"] = round(timed(enc_per_row, sync, args.warmup, iters) * 1e6, 1)
                row["b_data_gb_per_s"] = round(n / row["b_rows_us"] / 1e3, 2)
                print(json.dumps(row), flush=True)

                # decode: the text just made; the floor decodes as many symbols in one flat buffer
                d_src = device_bytes(want)
                flat = device_bytes(base64.b64encode(data.tobytes()))
                bcap, rcap = g.base64_rows_max_bytes(tlen), g.base64_rows_max_rows(tlen)
                d_out = torch.zeros(bcap + 16, dtype=torch.uint8, device=dev)
                d_oends = torch.zeros(rcap + 1, dtype=torch.int32, device=dev)
                p_src, p_out, p_oends = pinned(tlen), pinned(bcap), pinned(4 * rcap)

                def dec_before():  # a
                    p_src[:tlen].copy_(d_src)
                    sync()
                    got, nrows = native.base64_rows_twin(1, p_src.data_ptr(), tlen, p_out.data_ptr(), bcap,
                                                         p_oends.data_ptr(), rcap)
                    d_out[:got].copy_(p_out[:got])
                    d_oends.view(torch.uint8)[:4 * nrows].copy_(p_oends[:4 * nrows])
                    sync()
                    return got, nrows

                def dec_rows():  # b
                    return g.device_base64_decode_rows([d_src.data_ptr()], [tlen], [d_out.data_ptr()], [bcap],
                                                       [d_oends.data_ptr()], [rcap], 0)[0]

                def dec_flat():  # c
                    return g.device_base64_decode([flat.data_ptr()], [flat.numel()], [d_out.data_ptr()], [bcap + 16], 0)[0]

                assert dec_before() == (n, rows) and d_out[:n].cpu().numpy().tobytes() == data.tobytes()
                d_out.zero_()
                d_oends.zero_()
                assert tuple(dec_rows()[:4]) == (n, rows, 1, 0)
                assert d_out[:n].cpu().numpy().tobytes() == data.tobytes()
                assert np.array_equal(d_oends[:rows].cpu().numpy().view(np.uint32), ends)
                row = {"run": run, "direction": "decode", "data_bytes": n, "row_bytes": width, "rows": rows,
                       "text_bytes": tlen,
                       "a_d2h_twin_h2d_us": round(timed(dec_before, sync, args.warmup, iters) * 1e6, 1),
                       "b_rows_us": round(timed(dec_rows, sync, args.warmup, iters) * 1e6, 1),
                       "c_flat_us": round(timed(dec_flat, sync, args.warmup, iters) * 1e6, 1)}
                row["b_data_gb_per_s"] = round(n / row["b_rows_us"] / 1e3, 2)
                print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes-ki", default="4,64,1024,16384,65536")
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--table", metavar="PROFILE")
    ap.add_argument("--only", choices=["rows"], help="measure the rows form alone")
    ap.add_argument("--max-flat-jobs", type=int, default=1 << 16, help="rows: most rows route d is run with")
    args = ap.parse_args()
    if args.only == "rows":
        if args.sizes_ki == ap.get_default("sizes_ki"):
            args.sizes_ki = "4,64,1024,65536"
        return rows_table(args.table) if args.table else rows_main(args)
    if args.table:
        return table(args.table)
    from brpc_amd import native
    lib = load_helper()
    sizes = [int(float(x) * 1024) for x in args.sizes_ki.split(",")]
    gpu = not args.cpu_only
    if gpu:
        import torch
        from brpc_amd.ops.json import base64_decode, base64_encode
        assert torch.cuda.is_available() and native.gpu.device_count() > 0, "this benchmark needs the GPU (or --cpu-only)"
        dev = torch.device("cuda", 0)
    b_wins, d_wins, ratios = {}, {}, {}
    for run in range(args.runs):
        for n in sizes:
            data = np.random.default_rng(n + run).integers(0, 256, n, dtype=np.uint8).tobytes()
            text = base64.b64encode(data)
            assert native.base64_encode(data) == text and native.base64_decode(text) == data
            for decode, direction, src, want in ((0, "encode", data, text), (1, "decode", text, data)):
                iters = iters_for(n, args.iters)
                t_a, t_b = host_pair(lib, decode, src, want, min(args.warmup, 2), iters)
                key = (direction, n)
                b_wins[key] = b_wins.get(key, 0) + (t_b < t_a)
                row = {"run": run, "direction": direction, "data_bytes": n, "text_bytes": len(text),
                       "a_bytewise_us": round(t_a * 1e6, 1), "b_twin_us": round(t_b * 1e6, 1),
                       "a_over_b": round(t_a / t_b, 2), "b_data_gb_per_s": round(n / t_b / 1e9, 2)}
                if gpu:
                    cap = len(want) + 3  # decode: the size before the padding is known
                    dsrc = torch.from_numpy(np.frombuffer(src, dtype=np.uint8).copy()).to(dev)
                    ddst = torch.zeros(cap + 16, dtype=torch.uint8, device=dev)
                    pin_in = torch.empty(len(src), dtype=torch.uint8).pin_memory()
                    pin_out = torch.empty(cap, dtype=torch.uint8).pin_memory()
                    hsrc = torch.from_numpy(np.frombuffer(src, dtype=np.uint8).copy())
                    moved = (len(src) + len(want)) // 2
                    ca, cb = (torch.empty(moved, dtype=torch.uint8, device=dev) for _ in range(2))
                    fn = native.gpu.device_base64_decode if decode else native.gpu.device_base64_encode
                    op = base64_decode if decode else base64_encode
                    sync = torch.cuda.synchronize
                    sync()

                    def before():  # c
                        pin_in.copy_(dsrc)
                        sync()
                        got = lib.base64_bw_host(decode, pin_in.data_ptr(), len(src), pin_out.data_ptr(), cap)
                        ddst[:got].copy_(pin_out[:got])
                        sync()
                        return got

                    def hbm(off):  # d, e
                        return fn([dsrc.data_ptr()], [len(src)], [ddst.data_ptr() + off], [cap], 0)[0]

                    def through():  # f
                        pin_in.copy_(hsrc)
                        out = op(pin_in.to(dev, non_blocking=True))
                        pin_out[:out.numel()].copy_(out)
                        sync()
                        return out.numel()

                    def copy():  # g
                        cb.copy_(ca)
                        sync()

                    # every path gives the same bytes
                    assert before() == len(want) and ddst[:len(want)].cpu().numpy().tobytes() == want
                    for off in (0, 1):
                        ddst.zero_()
                        sync()
                        assert tuple(hbm(off)[:2]) == (len(want), 0)
                        assert ddst[off:off + len(want)].cpu().numpy().tobytes() == want
                    assert through() == len(want) and pin_out[:len(want)].numpy().tobytes() == want
                    t_c = timed(before, sync, args.warmup, iters)
                    t_d = timed(lambda: hbm(0), sync, args.warmup, iters)
                    t_e = timed(lambda: hbm(1), sync, args.warmup, iters)
                    t_f = timed(through, sync, args.warmup, iters)
                    t_g = timed(copy, sync, args.warmup, iters)
                    d_wins[key] = d_wins.get(key, 0) + (t_d < t_c)
                    ratios.setdefault(key, []).append(t_g / t_d)
                    row.update({"c_d2h_twin_h2d_us": round(t_c * 1e6, 1), "d_hbm_us": round(t_d * 1e6, 1),
                                "e_hbm_dst_plus_1_us": round(t_e * 1e6, 1), "f_host_through_device_us": round(t_f * 1e6, 1),
                                "g_copy_us": round(t_g * 1e6, 1), "c_over_d": round(t_c / t_d, 2),
                                "d_data_gb_per_s": round(n / t_d / 1e9, 2), "d_over_g": round(t_g / t_d, 3)})
                print(json.dumps(row), flush=True)
    verdict = {"runs": args.runs,
               "b_faster_than_a_in_every_run": {"%s %d" % k: v == args.runs for k, v in sorted(b_wins.items())}}
    if gpu:
        verdict["d_faster_than_c_in_every_run"] = {"%s %d" % k: v == args.runs for k, v in sorted(d_wins.items())}
        verdict["d_over_g_median"] = {"%s %d" % k: round(statistics.median(v), 3) for k, v in sorted(ratios.items())}
    print(json.dumps(verdict))


if __name__ == "__main__":
    main()
