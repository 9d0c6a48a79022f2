"""What a JSON string body costs on text that lives in HBM: escape (text ->
quoted JSON string), unescape (body -> text) and the UTF-8 verdict, five ways:

  b  host twin        json::EscapeStringBody / EscapeStringRows /
                      UnescapeStringBody / Utf8FirstBad between two pinned
                      buffers (native.json_string_twin)
  c  what a handler with the text in HBM had before: D2H into pinned memory,
                      the host twin, H2D of its result (validate: D2H + twin)
  d  device, HBM -> HBM   native.gpu.device_json_escape / _unescape /
                      device_utf8_validate, dst 16-byte aligned
  e  the same with dst off by one byte (validate: src off by one)
  g  a torch device copy that moves as many bytes as d does (half of what it
                      reads plus writes), the memory-bound yardstick

on three inputs: "plain" ASCII text, "esc3" with one newline or quote per 32
bytes (about 3% escapes), and for the escaper "rows32", the plain text as rows
of 32 bytes with their row_ends in HBM. Sizes are of the unescaped text. All
are timed on the host around the blocking call (g with a device synchronize),
--warmup untimed and a few timed calls, the median reported; GB/s is of text
bytes. The sweep repeats --runs times. Prints one JSON line per entry, input,
size and run, then whether d beat c in every run and d against g.

The entry "unescape_rows" (--only rows, or after the others) is the text of an
array of strings, ["r0","r1",...], back into bytes and row ends
(native.gpu.device_json_unescape_rows), on plain and esc3 text cut into rows of
32 and of 1024 bytes:

  a  what a handler had before: D2H, json::Reader, a concatenation of its
                      strings with their row ends, H2D of both
  b  host twin        json::UnescapeStringRows between pinned buffers
  c  D2H + b + H2D of bytes and row ends
  d  device, HBM -> HBM
  g  a torch device copy of as many bytes as d moves

  python benchmarks/json_string_bw.py [--sizes-ki 4,64,1024,16384,65536] [--runs 3] [--only bodies|rows]
  python benchmarks/json_string_bw.py --table profiles/json_string.txt   # the README table
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def iters_for(n, iters):
    return iters if n <= (1 << 20) else max(3, iters // 3)


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


def make_text(n, kind, seed):
    rng = np.random.default_rng(seed)
    text = rng.integers(ord("a"), ord("z") + 1, n, dtype=np.uint8)
    text[rng.integers(0, n, n // 6)] = ord(" ")
    if kind == "esc3":
        at = np.arange(0, n, 32) + rng.integers(0, 32, (n + 31) // 32)
        at = at[at < n]
        text[at] = np.where(rng.integers(0, 2, at.size) == 0, ord("\n"), ord('"')).astype(np.uint8)
    return text.tobytes()


def table(path):
    """The README table from a profile: medians over the runs found there."""
    rows = {}
    for line in open(path):
        line = line.strip()
        if not line.startswith('{"run"'):
            continue
        r = json.loads(line)
        rows.setdefault((r["entry"], r["input"], r["text_bytes"]), []).append(r)
    order = {"escape": 0, "unescape": 1, "validate": 2}
    rows_entry = {k: v for k, v in rows.items() if k[0] == "unescape_rows"}
    rows = {k: v for k, v in rows.items() if k[0] != "unescape_rows"}
    if rows_entry:
        print("| input | text | a D2H + reader + H2D | b host twin | c D2H + b + H2D | d device | d GB/s | a / d | c / d | d / g |")
        print("|---|---|---|---|---|---|---|---|---|---|")
        for (entry, kind, n), rs in sorted(rows_entry.items(), key=lambda kv: (kv[0][1], kv[0][2])):
            def span(k):
                v = [r[k] for r in rs]
                return "%.1f µs (%.1f–%.1f)" % (statistics.median(v), min(v), max(v))

            def mid(k):
                return statistics.median(r[k] for r in rs)
            name = "%d KiB" % (n >> 10) if n < 1 << 20 else "%d MiB" % (n >> 20)
            print("| %s | %s | %s | %s | %s | %s | %.2f | %.1f | %.2f | %.2f |" % (
                kind, name, span("a_d2h_reader_h2d_us"), span("b_twin_us"), span("c_d2h_twin_h2d_us"), span("d_hbm_us"),
                mid("d_text_gb_per_s"), mid("a_over_d"), mid("c_over_d"), mid("d_over_g")))
        if not rows:
            return
    print("| entry | input | text | b host twin | c D2H + b + H2D | d device | e device, + 1 | d GB/s | c / d | d / g |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for (entry, kind, n), rs in sorted(rows.items(), key=lambda kv: (order[kv[0][0]], kv[0][1], kv[0][2])):
        def med(k):
            return statistics.median(r[k] for r in rs)
        name = "%d KiB" % (n >> 10) if n < 1 << 20 else "%d MiB" % (n >> 20)
        print("| %s | %s | %s | %.1f µs | %.1f µs | %.1f µs | %.1f µs | %.1f | %.1f | %.2f |" % (
            entry, kind, name, med("b_twin_us"), med("c_d2h_twin_h2d_us"), med("d_hbm_us"), med("e_hbm_plus_1_us"),
            med("d_text_gb_per_s"), med("c_over_d"), med("d_over_g")))


def rows_sweep(args, torch, native, dev, sizes):
    """The entry unescape_rows: see the module docstring."""
    sync = torch.cuda.synchronize
    d_wins, ratios = {}, {}
    for run in range(args.runs):
        for n in sizes:
            for kind in ("plain", "esc3"):
                for row in (32, 1024):
                    text = make_text(n, kind, n + run)
                    ends = np.minimum(np.arange(row, n + row, row, dtype=np.int64), n).astype(np.uint32)
                    src = b"[" + native.json_escape(text, row_ends=ends.tobytes()) + b"]"
                    nrows = ends.size
                    iters = iters_for(n, args.iters)
                    dsrc = torch.from_numpy(np.frombuffer(src, dtype=np.uint8).copy()).to(dev)
                    ddst = torch.zeros(n + 16, dtype=torch.uint8, device=dev)
                    dends = torch.zeros(nrows, dtype=torch.int32, device=dev)
                    pin_in = torch.empty(len(src), dtype=torch.uint8).pin_memory()
                    pin_out = torch.empty(n + 16, dtype=torch.uint8).pin_memory()
                    pin_ends = torch.empty(nrows, dtype=torch.int32).pin_memory()
                    moved = max((len(src) + n + 4 * nrows) // 2, 1)
                    ca, cb = (torch.empty(moved, dtype=torch.uint8, device=dev) for _ in range(2))
                    pin_in.copy_(dsrc)
                    sync()

                    def twin(op=3):  # b (op 4: through json::Reader)
                        return native.json_string_twin(op, pin_in.data_ptr(), len(src), pin_out.data_ptr(), n + 16,
                                                       pin_ends.data_ptr(), nrows)

                    def staged(op):  # a (op 4), c (op 3)
                        pin_in.copy_(dsrc)
                        sync()
                        got = twin(op)
                        ddst[:got].copy_(pin_out[:got])
                        dends.copy_(pin_ends)
                        sync()
                        return got

                    def hbm():  # d
                        return native.gpu.device_json_unescape_rows([dsrc.data_ptr()], [len(src)], [ddst.data_ptr()], [n],
                                                                    [dends.data_ptr()], [nrows], 0)[0]

                    def copy():  # g
                        cb.copy_(ca)
                        sync()

                    # every path gives the same bytes and row ends
                    for path in (lambda: staged(4), lambda: staged(3), hbm):
                        ddst.zero_()
                        dends.zero_()
                        sync()
                        got = path()
                        assert got == n or tuple(got) == (n, nrows, 1, 0, 0), got
                        assert ddst[:n].cpu().numpy().tobytes() == text
                        assert (dends.cpu().numpy().view(np.uint32) == ends).all()
                    t_a = timed(lambda: staged(4), sync, min(args.warmup, 2), iters)
                    t_b = timed(twin, lambda: None, min(args.warmup, 2), iters)
                    t_c = timed(lambda: staged(3), sync, args.warmup, iters)
                    t_d = timed(hbm, sync, args.warmup, iters)
                    t_g = timed(copy, sync, args.warmup, iters)
                    key = ("unescape_rows", "%s rows%d" % (kind, row), n)
                    d_wins[key] = d_wins.get(key, 0) + (t_d < t_c)
                    ratios.setdefault(key, []).append(t_g / t_d)
                    print(json.dumps({
                        "run": run, "entry": key[0], "input": key[1], "text_bytes": n, "src_bytes": len(src), "rows": nrows,
                        "a_d2h_reader_h2d_us": round(t_a * 1e6, 1), "b_twin_us": round(t_b * 1e6, 1),
                        "c_d2h_twin_h2d_us": round(t_c * 1e6, 1), "d_hbm_us": round(t_d * 1e6, 1),
                        "g_copy_us": round(t_g * 1e6, 1), "a_over_d": round(t_a / t_d, 2), "c_over_d": round(t_c / t_d, 2),
                        "d_text_gb_per_s": round(n / t_d / 1e9, 2), "d_over_g": round(t_g / t_d, 3)}), flush=True)
    print(json.dumps({
        "runs": args.runs,
        "d_faster_than_c_in_every_run": {"%s %s %d" % k: v == args.runs for k, v in sorted(d_wins.items())},
        "d_over_g_median": {"%s %s %d" % k: round(statistics.median(v), 3) for k, v in sorted(ratios.items())}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes-ki", default="4,64,1024,16384,65536")
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--table", metavar="PROFILE")
    ap.add_argument("--only", choices=("bodies", "rows"), help="bodies: escape / unescape / validate; rows: unescape_rows")
    args = ap.parse_args()
    if args.table:
        return table(args.table)
    import torch
    from brpc_amd import native
    assert torch.cuda.is_available() and native.gpu.device_count() > 0, "this benchmark needs the GPU"
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    sizes = [int(float(x) * 1024) for x in args.sizes_ki.split(",")]
    if args.only == "rows":
        return rows_sweep(args, torch, native, dev, sizes)
    cases = [("escape", "plain"), ("escape", "esc3"), ("escape", "rows32"), ("unescape", "plain"), ("unescape", "esc3"),
             ("validate", "plain"), ("validate", "esc3")]
    d_wins, ratios = {}, {}
    for run in range(args.runs):
        for n in sizes:
            for entry, kind in cases:
                text = make_text(n, "plain" if kind == "rows32" else kind, n + run)
                ends = None
                if kind == "rows32":
                    ends = np.minimum(np.arange(32, n + 32, 32, dtype=np.int64), n).astype(np.uint32)
                    quoted = native.json_escape(text, row_ends=ends.tobytes())
                else:
                    quoted = native.json_escape(text)
                op = {"escape": 0, "unescape": 1, "validate": 2}[entry]
                src, want = {0: (text, quoted), 1: (quoted[1:-1], text), 2: (text, b"")}[op]
                iters = iters_for(n, args.iters)
                cap = max(len(want), len(src)) + 16  # the unescaper asks for room for the whole body
                dsrc = torch.zeros(len(src) + 16, dtype=torch.uint8, device=dev)
                dsrc[:len(src)] = torch.from_numpy(np.frombuffer(src, dtype=np.uint8).copy()).to(dev)
                dsrc1 = torch.zeros(len(src) + 16, dtype=torch.uint8, device=dev)  # the same text one byte further
                dsrc1[1:len(src) + 1] = dsrc[:len(src)]
                ddst = torch.zeros(cap + 16, dtype=torch.uint8, device=dev)
                pin_in = torch.empty(len(src), dtype=torch.uint8).pin_memory()
                pin_out = torch.empty(cap, dtype=torch.uint8).pin_memory()
                pin_in.copy_(dsrc[:len(src)])
                dends = torch.from_numpy(ends.view(np.int32).copy()).to(dev) if ends is not None else None
                pends = torch.from_numpy(ends.view(np.int32).copy()).pin_memory() if ends is not None else None
                nrows = 0 if ends is None else ends.size
                moved = max((len(src) + len(want)) // 2, 1)
                ca, cb = (torch.empty(moved, dtype=torch.uint8, device=dev) for _ in range(2))
                sync()

                def twin():  # b
                    return native.json_string_twin(op, pin_in.data_ptr(), len(src), pin_out.data_ptr(), cap,
                                                   pends.data_ptr() if nrows else 0, nrows)

                def before():  # c
                    pin_in.copy_(dsrc[:len(src)])
                    sync()
                    got = twin()
                    if op != 2:
                        ddst[:got].copy_(pin_out[:got])
                        sync()
                    return got

                def hbm(off):  # d, e
                    if op == 0:
                        return native.gpu.device_json_escape([dsrc.data_ptr()], [len(src)], [ddst.data_ptr() + off], [cap],
                                                             [dends.data_ptr()] if nrows else [], [nrows] if nrows else [])[0]
                    if op == 1:
                        return native.gpu.device_json_unescape([dsrc.data_ptr()], [len(src)], [ddst.data_ptr() + off],
                                                               [cap], 0)[0]
                    return native.gpu.device_utf8_validate([(dsrc1.data_ptr() + 1) if off else dsrc.data_ptr()],
                                                           [len(src)], 0)[0]

                def copy():  # g
                    cb.copy_(ca)
                    sync()

                # every path gives the same bytes
                if op == 2:
                    assert before() == len(src) and hbm(0) == (0, 0) and hbm(1) == (0, 0)
                else:
                    assert before() == len(want) and ddst[:len(want)].cpu().numpy().tobytes() == want
                    for off in (0, 1):
                        ddst.zero_()
                        sync()
                        assert tuple(hbm(off)[:2]) == (len(want), 0)
                        assert ddst[off:off + len(want)].cpu().numpy().tobytes() == want
                t_b = timed(twin, lambda: None, min(args.warmup, 2), iters)
                t_c = timed(before, sync, args.warmup, iters)
                t_d = timed(lambda: hbm(0), sync, args.warmup, iters)
                t_e = timed(lambda: hbm(1), sync, args.warmup, iters)
                t_g = timed(copy, sync, args.warmup, iters)
                key = (entry, kind, n)
                d_wins[key] = d_wins.get(key, 0) + (t_d < t_c)
                ratios.setdefault(key, []).append(t_g / t_d)
                print(json.dumps({
                    "run": run, "entry": entry, "input": kind, "text_bytes": n, "src_bytes": len(src),
                    "dst_bytes": len(want), "b_twin_us": round(t_b * 1e6, 1), "c_d2h_twin_h2d_us": round(t_c * 1e6, 1),
                    "d_hbm_us": round(t_d * 1e6, 1), "e_hbm_plus_1_us": round(t_e * 1e6, 1),
                    "g_copy_us": round(t_g * 1e6, 1), "c_over_d": round(t_c / t_d, 2),
                    "d_text_gb_per_s": round(n / t_d / 1e9, 2), "d_over_g": round(t_g / t_d, 3)}), flush=True)
    print(json.dumps({
        "runs": args.runs,
        "d_faster_than_c_in_every_run": {"%s %s %d" % k: v == args.runs for k, v in sorted(d_wins.items())},
        "d_over_g_median": {"%s %s %d" % k: round(statistics.median(v), 3) for k, v in sorted(ratios.items())}}))
    if args.only is None:
        rows_sweep(args, torch, native, dev, sizes)


if __name__ == "__main__":
    main()
