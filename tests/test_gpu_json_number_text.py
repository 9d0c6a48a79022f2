"""JSON number text parsed on the device with no separator table
(gpu::DeviceParseNumberText; json_text_count_kernel / json_text_parse_kernel
in gpu/json_kernels.hip) and the ops on top of it. Everything is compared
byte for byte with the host twin native.json_parse_number_text, which
tests/test_json_number_text.py pins to Python's float() and json.loads and
brpc_amd/csrc/tests/number_text_unittest.cc to its refusals."""
import json
import math
import random
import struct
from fractions import Fraction

import pytest

torch = pytest.importorskip("torch")
np = pytest.importorskip("numpy")
pytestmark = pytest.mark.gpu

NUMBERS, FLOAT64, FLOAT32 = 0, 1, 2
INT64, UINT64, DOUBLE, NEEDS_EXACT = 0, 1, 2, 3
NONE = 0xFFFFFFFF
E25 = "-1.2345678901234567e-0006"  # the longest element of _mixed


@pytest.fixture(scope="module")
def dev():
    from brpc_amd import native
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert native.gpu.device_count() > 0, "native runtime sees no HIP device"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def C(native):
    c = native.gpu.json_text_chunk_bytes()
    assert c >= 256
    return c


def _mixed(n, seed=0):
    """Elements of 1 to 25 characters side by side, every class among them
    (the pattern of tests/test_gpu_json_float_parse.py)."""
    pattern = ["1", E25, "0.5", "-0", "1e300", "18446744073709551615", "2.5E+0", "-0.0",
               "123456.0", "9223372036854775807", "4.9e-324", "0.1234567890123456789", "-7", "1e22", "3.4028235e38",
               "-9223372036854775808", "1.7976931348623157e308", "6", "1e-400", "0.000001"]
    rng = random.Random(seed)
    out = [pattern[i % len(pattern)] for i in range(n)]
    for i in range(0, n, 7):
        out[i] = repr(rng.gauss(0.0, 1.0))
    assert max(len(t) for t in pattern) == 25 and min(len(t) for t in pattern) == 1
    return out


def _filler(r):
    """One element of exactly r >= 1 characters that a lane decides."""
    return "7" * r if r <= 18 else "0." + "0" * (r - 3) + "5"


def _of_length(length, seed=0):
    """Bare mixed text of exactly `length` >= 50 bytes."""
    elems, size = [], 0
    for e in _mixed(length, seed):
        if size + len(e) + 1 + 20 > length:  # the filler stays below the 48 characters a lane reads
            break
        elems.append(e)
        size += len(e) + 1
    elems.append(_filler(length - size))
    text = ",".join(elems)
    assert len(text) == length
    return text


def _nest(elems, sizes):
    rows, i, k = [], 0, 0
    while i < len(elems):
        rows.append(elems[i:i + sizes[k % len(sizes)]])
        i += len(rows[-1])
        k += 1
    return "[" + ",".join("[" + ",".join(r) + "]" for r in rows) + "]"


WIDTH = {NUMBERS: 8, FLOAT64: 8, FLOAT32: 4}


def _job(text, mode, cap=None, row_cap=None, redo_cap=8, nested=True, shift=0, out_shift=0):
    if isinstance(text, str):
        text = text.encode()
    return dict(text=text, mode=mode, cap=cap, row_cap=row_cap, redo_cap=redo_cap, nested=nested, shift=shift,
                out_shift=out_shift)


def _run(native, dev, jobs):
    """All jobs in one call. cap / row_cap default to what the twin says the
    text holds. Every buffer is filled with a sentinel first and comes back
    whole: out as bytes (cap elements), classes, row_ends and redo as arrays."""
    keep, args = [], [[] for _ in range(10)]
    for j in jobs:
        twin = native.json_parse_number_text(j["text"], j["mode"], False, j["nested"])
        cap = twin[2] if j["cap"] is None else j["cap"]
        row_cap = (twin[3] if j["nested"] else 0) if j["row_cap"] is None else j["row_cap"]
        raw = np.frombuffer(b"\xA5" * j["shift"] + j["text"], dtype=np.uint8).copy()
        t = torch.from_numpy(raw).to(dev) if len(raw) else torch.empty(0, dtype=torch.uint8, device=dev)
        w = WIDTH[j["mode"]]
        out = torch.full((cap * w + j["out_shift"] + 16,), 0x5A, dtype=torch.uint8, device=dev)
        cls = torch.full((cap + 1,), 0xEE, dtype=torch.uint8, device=dev)
        rows = torch.full((row_cap + 1,), -1, dtype=torch.int32, device=dev)
        redo = torch.full((2 * j["redo_cap"] + 2,), -1, dtype=torch.int32, device=dev)
        assert out.data_ptr() % 16 == 0
        keep.append((t, out, cls, rows, redo, cap, row_cap, twin))
        vals = [t.data_ptr() + j["shift"] if len(raw) else 0, len(j["text"]), j["mode"], out.data_ptr() + j["out_shift"],
                cls.data_ptr() if j["mode"] == NUMBERS else 0, cap, rows.data_ptr() if j["nested"] else 0, row_cap,
                redo.data_ptr() if j["redo_cap"] else 0, j["redo_cap"]]
        for lst, v in zip(args, vals):
            lst.append(v)
    torch.cuda.synchronize(dev)
    res = native.gpu.device_json_parse_text(*args, 0)
    outs = []
    for (err, depth, count, nrows, n_redo, bad), j, (t, out, cls, rows, redo, cap, row_cap, twin) in zip(res, jobs, keep):
        w = WIDTH[j["mode"]]
        o = out.cpu().numpy()
        assert bytes(o[:j["out_shift"]]) == b"\x5A" * j["out_shift"]
        assert bytes(o[j["out_shift"] + cap * w:]) == b"\x5A" * 16, "a store beyond cap"
        c = cls.cpu().numpy()
        assert c[cap] == 0xEE, "a class beyond cap"
        r = rows.cpu().numpy()
        assert r[row_cap] == -1, "a row end beyond row_cap"
        rd = redo.cpu().numpy().view(np.uint32)
        assert tuple(rd[2 * j["redo_cap"]:]) == (NONE, NONE), "a redo pair beyond redo_cap"
        outs.append(dict(err=err, depth=depth, count=count, rows=nrows, n_redo=n_redo, bad=bad,
                         out=o[j["out_shift"]:j["out_shift"] + cap * w].tobytes(), cls=c[:cap], row_ends=r[:row_cap],
                         redo=rd[:2 * j["redo_cap"]].reshape(-1, 2), twin=twin, job=j))
    return outs


def _same_as_twin(res):
    """A parsed job: verdict, values, classes and row ends are the twin's
    (the inexact twin's: elements it lists as class 3 are the redo list)."""
    j = res["job"]
    err, depth, count, rows, bad, out, classes, row_ends = res["twin"]
    assert err == 0, "the test's text is malformed"
    assert (res["err"], res["depth"], res["count"], res["rows"], res["bad"]) == (0, depth, count, rows, NONE), res
    w = WIDTH[j["mode"]]
    assert len(res["out"]) == count * w == len(out)
    if res["n_redo"] == 0:
        assert res["out"] == out
    else:
        listed = set(int(i) for i in res["redo"][:res["n_redo"], 0])
        for i in range(count):
            want = b"\x5A" * w if i in listed else out[i * w:i * w + w]  # nothing is written for a listed one
            assert res["out"][i * w:i * w + w] == want, i
    if j["mode"] == NUMBERS:
        want = bytes(0xEE if c == NEEDS_EXACT else c for c in classes)
        assert res["cls"].tobytes() == want
    else:
        assert bool((res["cls"] == 0xEE).all())  # typed modes write no classes
    if j["nested"]:
        assert [int(x) for x in res["row_ends"]] == row_ends


def _same_refusal(res):
    err, _, count, _, bad, _, _, _ = res["twin"]
    assert err == 1, "the test's text is not malformed"
    assert (res["err"], res["bad"], res["count"]) == (1, bad, count), res


@pytest.mark.parametrize("mode", [NUMBERS, FLOAT64, FLOAT32])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 769])
def test_counts_and_mixed_lengths(native, dev, mode, n):
    bare = ",".join(_mixed(n, seed=n))
    flat, bracketed = _run(native, dev, [_job(bare, mode), _job("[" + bare + "]", mode)])
    _same_as_twin(flat)
    _same_as_twin(bracketed)
    assert (flat["depth"], bracketed["depth"], flat["count"], bracketed["count"], flat["n_redo"]) == (0, 1, n, n, 0)
    assert flat["out"] == bracketed["out"]
    if mode == FLOAT64:
        assert flat["out"] == np.array([0.0 if e == "-0" else float(e) for e in _mixed(n, seed=n)]).tobytes()


def test_texts_around_the_chunk_size(native, dev, C):
    jobs = [_job(_of_length(length, seed=length), mode)
            for length in (C - 1, C, C + 1, 2 * C + 1) for mode in (NUMBERS, FLOAT64, FLOAT32)]
    jobs += [_job("[" + _of_length(length - 2, seed=length) + "]", FLOAT64) for length in (C - 1, C, C + 1, 2 * C + 1)]
    for res in _run(native, dev, jobs):
        _same_as_twin(res)
        assert res["count"] > 100 and res["n_redo"] == 0


def test_commas_and_elements_on_chunk_edges(native, dev, C):
    tail = "," + ",".join(_mixed(40, seed=4))
    last = _of_length(C - 1, seed=1) + tail   # a comma as the last byte of chunk 0
    first = _of_length(C, seed=2) + tail      # a comma as the first byte of chunk 1
    assert last[C - 1] == "," and first[C] == ","
    jobs = [_job(last, NUMBERS), _job(first, NUMBERS), _job(last, FLOAT32), _job(first, FLOAT64)]
    # a 25-character element straddling the edge at every split position
    for split in range(1, len(E25)):
        text = _of_length(C - split - 1, seed=split) + "," + E25 + tail
        assert text[C - split:C - split + len(E25)] == E25 and text[C - split - 1] == ","
        jobs.append(_job(text, NUMBERS if split % 2 else FLOAT64))
    for res in _run(native, dev, jobs):
        _same_as_twin(res)
        assert res["n_redo"] == 0


@pytest.mark.parametrize("shift", [1, 3, 15])
def test_any_text_alignment_and_the_minimum_of_out(native, dev, C, shift):
    text = "[" + _of_length(C + 300, seed=shift) + "]"
    for res in _run(native, dev, [_job(text, NUMBERS, shift=shift, out_shift=8), _job(text, FLOAT64, shift=shift, out_shift=8),
                                  _job(text, FLOAT32, shift=shift, out_shift=4), _job(text, FLOAT32, shift=shift, out_shift=12)]):
        _same_as_twin(res)


def test_whitespace_of_every_kind(native, dev, C):
    elems = _mixed(3 * C // 80, seed=8)
    kinds = [" ", "\t", "\n", "\r"]
    every = " \t[\r\n" + ",".join(kinds[i % 4] + e + kinds[(i + 1) % 4] + kinds[(i + 2) % 4] for i, e in enumerate(elems)) + "\n]\t \r"
    padded = ",".join(" " * 80 + e for e in elems)       # a chunk holds few pieces
    both = "[ " + " , ".join(" " * 40 + e + " " * 40 for e in elems) + " ]"
    hole = "1.5," + " " * (2 * C) + "2.5"                # an all-whitespace chunk between two elements
    hole_in = "[ 1.5" + "\n" * (2 * C) + ",\t2.5" + "\r" * C + "]"
    assert len(padded) > 3 * C
    for res in _run(native, dev, [_job(every, NUMBERS), _job(padded, FLOAT64), _job(both, FLOAT32), _job(hole, FLOAT64),
                                  _job(hole_in, NUMBERS), _job(" \t\r\n" * C, FLOAT64), _job("  [\n]\t", FLOAT32)]):
        _same_as_twin(res)
    res = _run(native, dev, [_job(hole, FLOAT64)])[0]
    assert res["out"] == struct.pack("<2d", 1.5, 2.5)


@pytest.mark.parametrize("sizes", [[1], [3], [300], [1, 5, 2, 64, 3]])
def test_rows(native, dev, C, sizes):
    elems = _mixed(3 * C // 10, seed=sum(sizes))
    text = _nest(elems, sizes)
    assert len(text) > 2 * C
    spaced = text.replace("],[", " ]\n,\t[ ")
    results = _run(native, dev, [_job(text, m) for m in (NUMBERS, FLOAT64, FLOAT32)] + [_job(spaced, FLOAT64)])
    for res in results:
        _same_as_twin(res)
        assert res["depth"] == 2 and res["count"] == len(elems)
    want = np.cumsum([len(r) for r in json.loads(text)])
    assert [int(x) for x in results[1]["row_ends"]] == list(want)


def test_row_boundaries_on_a_chunk_edge_and_small_nested_texts(native, dev, C):
    tail = "],[" + "],[".join(",".join(_mixed(5, seed=s)) for s in range(30)) + "]]"
    jobs = []
    for k in range(-1, 4):  # the ']' of "],[" at C - 3 .. C + 1: the edge before, inside and after the three bytes
        head = "[[" + _of_length(C - 2 - 2 + k, seed=k + 2)
        text = head + tail
        assert text[C - 2 + k:C + 1 + k] == "],["
        jobs.append(_job(text, FLOAT64))
        jobs.append(_job(text.replace("],[", "] , ["), NUMBERS))
    jobs += [_job("[[1,2]]", FLOAT64), _job("[[7]]", FLOAT32), _job(" [ [1] , [2,3] ] ", NUMBERS)]
    results = _run(native, dev, jobs)
    for res in results:
        _same_as_twin(res)
        assert res["depth"] == 2
    assert (results[-3]["rows"], [int(x) for x in results[-3]["row_ends"]]) == (1, [2])
    assert (results[-1]["rows"], [int(x) for x in results[-1]["row_ends"]]) == (2, [1, 3])
    # nowhere to put row ends: nested text is malformed at piece 0
    for res in _run(native, dev, [_job("[[1,2]]", FLOAT64, nested=False), _job(jobs[0]["text"], FLOAT64, nested=False)]):
        assert (res["err"], res["bad"]) == (1, 0)
        _same_refusal(res)


def _index_at(elems, pos):
    """The element of ','.join(elems) that holds byte `pos`."""
    at = 0
    for i, e in enumerate(elems):
        at += len(e) + 1
        if at > pos:
            return i
    raise AssertionError


def test_refusals_name_the_lowest_piece(native, dev, C):
    elems = _mixed(3 * C // 10, seed=6)
    assert len(",".join(elems)) > 2 * C + 100
    edge, last = _index_at(elems, C), len(elems) - 1
    assert 0 < edge < _index_at(elems, 2 * C) < last
    jobs = []
    for at in (3, edge - 1, edge, edge + 1, last):
        for junk in ("1.", '"NaN"', "", "1 2", "[2]", "2]"):
            bad = list(elems)
            bad[at] = junk
            jobs.append((at, _job(",".join(bad), FLOAT64)))
            jobs.append((at, _job("[" + ",".join(bad) + "]", NUMBERS)))
    results = _run(native, dev, [j for _, j in jobs])
    for (at, _), res in zip(jobs, results):
        _same_refusal(res)
        assert res["bad"] == at, res["job"]["text"][:40]
    # two bad pieces: the lower index, whichever chunk finishes first
    two = list(elems)
    two[edge + 1], two[last - 2] = "1.", '"NaN"'
    bare = ",".join(elems)
    shapes = [",".join(two), bare + ",", "[" + bare + ",]", bare + "," * C + bare, "," * C, "[" + bare, bare + "]",
              "[" + bare + "]]", "[[" + bare + "]", "[1,[2]]", "[[1][2]]", "[[],[1]]", "[[[1]]]", "[[1],[]]", "[[1],2]",
              "[1],[2]", _nest(elems, [7])[:-1], _nest(elems, [7]) + "]", _nest(elems, [7]).replace("],[", "][", 1),
              _nest(elems, [7])[1:], "[" + bare + "] x", "x", "[1,2]\x00"]
    results = _run(native, dev, [_job(t, FLOAT64) for t in shapes])
    for res in results:
        _same_refusal(res)
    assert results[0]["bad"] == edge + 1 and results[1]["bad"] == len(elems) and results[3]["bad"] == len(elems)
    assert [r["bad"] for r in results[9:13]] == [1, 0, 0, 0]


def test_capacity(native, dev, C):
    elems = _mixed(3 * C // 10, seed=11)
    n = len(elems)
    flat, nested = ",".join(elems), _nest(elems, [9])
    rows = (n + 8) // 9
    short, exact, rows_short, rows_exact, none = _run(native, dev, [
        _job(flat, FLOAT64, cap=n - 1), _job(flat, NUMBERS, cap=n), _job(nested, FLOAT32, cap=n, row_cap=rows - 1),
        _job(nested, FLOAT64, cap=n, row_cap=rows), _job(flat, FLOAT64, cap=0)])
    # _run has checked the sentinels past cap, row_cap and redo_cap
    assert (short["err"], short["count"], short["bad"]) == (5, n, NONE)
    assert short["out"] == short["twin"][5][:8 * (n - 1)]  # what fits is there
    _same_as_twin(exact)
    assert (rows_short["err"], rows_short["count"], rows_short["rows"]) == (5, n, rows)
    assert [int(x) for x in rows_short["row_ends"]] == rows_short["twin"][7][:rows - 1]
    _same_as_twin(rows_exact)
    assert (none["err"], none["count"]) == (5, n)


def _three_undecided(native):
    """Three 30-digit numbers the twin reports as needing exact arithmetic:
    the search of tests/test_gpu_json_float_parse.py."""
    found = []
    rng = random.Random(30)
    while len(found) < 3:
        d = struct.unpack("<d", struct.pack("<Q", rng.getrandbits(62) | (1 << 61)))[0]
        if not (1e-300 < d < 1e300):
            continue
        mid = (Fraction(d) + Fraction(math.nextafter(d, math.inf))) / 2
        e10 = math.floor(math.log10(d))
        digits = str(int(mid * Fraction(10) ** (29 - e10)))
        if len(digits) != 30:
            continue
        t = "%s.%se%d" % (digits[0], digits[1:], e10)
        if native.json_parse_numbers(t.encode(), False)[1][0] == NEEDS_EXACT:
            found.append(t)
    return found


def _redo_text(native, C):
    """Shortest-printed normals (no redo among them) with four undecided
    elements in different chunks: (elements, their indices)."""
    a = np.random.default_rng(12).standard_normal(3 * C // 10)
    elems = native.json_format_floats(a.tobytes(), 9).decode().split(",")
    assert NEEDS_EXACT not in set(native.json_parse_number_text(",".join(elems).encode(), NUMBERS, False)[6])
    longer = "0." + "3" * native.json_max_device_number_chars()
    where = [2, _index_at(elems, C + 50), _index_at(elems, 2 * C + 50), len(elems) - 1]
    for i, t in zip(where, _three_undecided(native) + [longer]):
        elems[i] = t
    return elems, where


def test_redo_pairs(native, dev, C):
    elems, where = _redo_text(native, C)
    for text in (",".join(elems), " [\n" + " , ".join(elems) + "]", _nest(elems, [11])):
        for mode in (NUMBERS, FLOAT64):
            res, small, none = _run(native, dev, [_job(text, mode), _job(text, mode, redo_cap=2), _job(text, mode, redo_cap=0)])
            assert res["n_redo"] == 4
            _same_as_twin(res)
            pairs = sorted((int(i), int(off)) for i, off in res["redo"][:4])
            assert [i for i, _ in pairs] == where
            for i, off in pairs:  # the offset is the byte after the separator, and the piece holds the element
                assert off == 0 or text[off - 1] == ","
                assert text[off:].lstrip(" \t\r\n[").startswith(elems[i])
            assert (small["err"], small["n_redo"], small["bad"]) == (3, 4, NONE)
            assert set(int(i) for i in small["redo"][:, 0]) <= set(where)
            assert (none["err"], none["n_redo"]) == (3, 4)


def test_refused_before_any_launch(native, dev):
    text = torch.from_numpy(np.frombuffer(b"1.5,2.5", dtype=np.uint8).copy()).to(dev)
    out = torch.full((64,), 0xEE, dtype=torch.uint8, device=dev)
    side = torch.full((64,), 0xEE, dtype=torch.uint8, device=dev)

    def code(mode, out_ptr, cls_ptr=0, text_ptr=None, n=7, cap=2, rows_ptr=0, row_cap=0, redo_ptr=0, redo_cap=0):
        (err, depth, count, rows, n_redo, bad), = native.gpu.device_json_parse_text(
            [text.data_ptr() if text_ptr is None else text_ptr], [n], [mode], [out_ptr], [cls_ptr], [cap], [rows_ptr],
            [row_cap], [redo_ptr], [redo_cap], 0)
        if err == 2:
            assert (depth, count, rows, n_redo, bad) == (0, 0, 0, 0, NONE)
        return err

    assert code(FLOAT64, 0) == 2                                   # null out
    assert code(3, out.data_ptr(), side.data_ptr()) == 2           # bad mode
    assert code(FLOAT64, out.data_ptr() + 4) == 2                  # misaligned for a double
    assert code(FLOAT32, out.data_ptr() + 2) == 2                  # misaligned for a float
    assert code(NUMBERS, out.data_ptr()) == 2                      # numbers without classes
    assert code(FLOAT64, out.data_ptr(), text_ptr=0) == 2          # null text
    assert code(FLOAT64, out.data_ptr(), n=(1 << 32) - 1) == 2     # too large
    assert code(FLOAT64, out.data_ptr(), redo_cap=4) == 2          # redo_cap without redo
    assert code(FLOAT64, out.data_ptr(), row_cap=4) == 2           # row_cap without row_ends
    assert code(FLOAT64, out.data_ptr(), rows_ptr=side.data_ptr() + 2, row_cap=4) == 2
    assert code(FLOAT64, out.data_ptr(), redo_ptr=side.data_ptr() + 2, redo_cap=4) == 2
    torch.cuda.synchronize(dev)
    assert bool((out == 0xEE).all()) and bool((side == 0xEE).all())
    assert code(FLOAT64, out.data_ptr()) == 0
    assert bytes(out[:16].cpu().numpy()) == struct.pack("<2d", 1.5, 2.5)
    assert code(FLOAT64, out.data_ptr(), n=0) == 0                 # empty: nothing to parse
    assert code(FLOAT64, 0, text_ptr=0, n=0, cap=0) == 0


def test_jobs_of_every_kind_in_one_call(native, dev, C):
    elems = _mixed(2 * C // 10, seed=13)
    bad = list(elems)
    bad[len(bad) // 2] = "1e"
    a, b, c, d, e = _run(native, dev, [_job(",".join(elems), NUMBERS), _job("[" + ",".join(bad) + "]", FLOAT64),
                                       _job("", FLOAT32), _job(_nest(elems, [4]), FLOAT32),
                                       _job("[" + ",".join(elems[:70]) + "]", FLOAT64)])
    _same_as_twin(a)
    _same_refusal(b)
    assert b["bad"] == len(bad) // 2
    assert (c["err"], c["count"], c["depth"]) == (0, 0, 0)
    _same_as_twin(d)
    _same_as_twin(e)
    assert (a["depth"], d["depth"], e["depth"]) == (0, 2, 1)


def _device_text(dev, text):
    return torch.from_numpy(np.frombuffer(text if isinstance(text, bytes) else text.encode(), dtype=np.uint8).copy()).to(dev)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_ops_round_trip_the_printer(native, dev, dtype):
    from brpc_amd import ops
    rng = np.random.default_rng(14)
    a = rng.standard_normal((8, 257)).astype(dtype)
    a[3, 5], a[7, 256] = 0.0, np.finfo(dtype).tiny
    t = torch.from_numpy(a).to(dev)
    flat = ops.json_print_floats(t)
    back = ops.json_parse_floats(flat, dtype=t.dtype)
    assert back.dtype == t.dtype and back.cpu().numpy().tobytes() == a.tobytes()
    spaced = _device_text(dev, b" [ " + bytes(flat.cpu().numpy()) + b"\n]\n")
    assert ops.json_parse_floats(spaced, dtype=t.dtype).cpu().numpy().tobytes() == a.tobytes()
    assert ops.json_parse_floats(flat, dtype=t.dtype, max_elems=a.size).cpu().numpy().tobytes() == a.tobytes()
    with pytest.raises(ValueError, match="max_elems"):
        ops.json_parse_floats(flat, dtype=t.dtype, max_elems=a.size - 1)
    # printed row by row
    rows = [bytes(ops.json_print_floats(t[r]).cpu().numpy()) for r in range(8)]
    nested = _device_text(dev, b"[[" + b"],[".join(rows) + b"]]")
    back = ops.json_parse_float_rows(nested, dtype=t.dtype)
    assert back.shape == (8, 257) and back.dtype == t.dtype and back.cpu().numpy().tobytes() == a.tobytes()
    ragged = _device_text(dev, b"[[" + b"],[".join(rows[:2]) + b"],[" + rows[2][:rows[2].rindex(b",")] + b"],[" + rows[3] + b"]]")
    with pytest.raises(ValueError, match="row 2 has 256 elements, row 0 has 257"):
        ops.json_parse_float_rows(ragged, dtype=t.dtype)
    values, ends = ops.json_parse_float_rows(ragged, dtype=t.dtype, ragged=True)
    assert ends.tolist() == [257, 514, 770, 1027] and ends.dtype == torch.int64
    want = np.concatenate([a[0], a[1], a[2][:256], a[3]])
    assert values.cpu().numpy().tobytes() == want.tobytes()
    assert ops.json_parse_float_rows(_device_text(dev, "[ ]")).shape == (0, 0)
    with pytest.raises(ValueError, match="not an array of arrays"):
        ops.json_parse_float_rows(_device_text(dev, "[1,2]"))
    with pytest.raises(ValueError, match="element 0 "):
        ops.json_parse_floats(nested)  # the flat op takes no rows
    with pytest.raises(ValueError, match="element 3 "):
        ops.json_parse_float_rows(_device_text(dev, "[[1,2],[3,[4]]]"))


def test_ops_repair_redo_elements(native, dev, C):
    from brpc_amd import ops
    elems, where = _redo_text(native, C)
    want = np.array([float(e) for e in elems])
    got = ops.json_parse_floats(_device_text(dev, " [ " + " ,".join(elems) + " ] "))
    assert got.cpu().numpy().tobytes() == want.tobytes()
    with np.errstate(all="ignore"):
        got = ops.json_parse_floats(_device_text(dev, ",".join(elems)), dtype=torch.float32)
        assert got.cpu().numpy().tobytes() == want.astype(np.float32).tobytes()
    rows = ops.json_parse_float_rows(_device_text(dev, _nest(elems[:len(elems) // 12 * 12] + [elems[-1]] * 12, [12])))
    assert rows.shape[1] == 12 and rows.cpu().numpy().tobytes() == np.concatenate([want[:len(elems) // 12 * 12], [want[-1]] * 12]).tobytes()
    # more undecided elements than the first list holds: the call is repeated with room for all
    many = ",".join(_three_undecided(native) * 30)
    got = ops.json_parse_floats(_device_text(dev, many))
    assert got.cpu().numpy().tobytes() == np.array([float(e) for e in many.split(",")]).tobytes()


def _balanced(native, call, calls=50):
    """As tests/test_gpu_pool_balance.py: after a warm-up, 50 calls leave the pool as it was."""
    call()
    before = native.gpu.hbm_pool_stats(0)
    for _ in range(calls):
        call()
    after = native.gpu.hbm_pool_stats(0)
    assert after["live_blocks"] == before["live_blocks"], (before, after)
    assert after["live_bytes"] == before["live_bytes"], (before, after)
    assert after["pinned_bytes"] <= before["pinned_bytes"], (before, after)


@pytest.mark.parametrize("path", ["parsed", "declined"])
def test_pool_balance(native, dev, C, path):
    elems = _mixed(C // 5, seed=15)
    if path == "declined":
        elems[len(elems) // 2] = '"NaN"'
    raw = ("[" + ",".join(elems) + "]").encode()
    text = _device_text(dev, raw)
    out = torch.empty(len(elems), dtype=torch.float64, device=dev)
    want = native.json_parse_number_text(raw, FLOAT64)
    torch.cuda.synchronize(dev)

    def call():
        (err, depth, count, rows, n_redo, bad), = native.gpu.device_json_parse_text(
            [text.data_ptr()], [len(raw)], [FLOAT64], [out.data_ptr()], [0], [len(elems)], [0], [0], [0], [0], 0)
        assert (err, bad) == (want[0], want[4])

    _balanced(native, call)
    if path == "parsed":
        assert out.cpu().numpy().tobytes() == want[5]
