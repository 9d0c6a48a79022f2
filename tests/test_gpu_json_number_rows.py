"""Number arrays and nested number rows printed as JSON text on the device
(gpu::DevicePrintNumbers; json_number_size_kernel / json_number_rows_kernel /
json_number_place_kernel), and the integer parsers of ops.json that read the
text back. Every text is compared byte for byte with the host twin
native.json_format_number_rows, which tests/test_json_number_rows_host.py pins
to Python's json module and brpc_amd/csrc/tests/number_print_unittest.cc to a
naive printer."""
import pytest

torch = pytest.importorskip("torch")
np = pytest.importorskip("numpy")
pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
SENTINEL = 0xA5
INT32, UINT32, SINT32, INT64, UINT64, SINT64, BOOL, FLOAT, DOUBLE = 0, 1, 2, 3, 4, 5, 6, 8, 9
DTYPES = {INT32: np.int32, UINT32: np.uint32, SINT32: np.int32, INT64: np.int64, UINT64: np.uint64, SINT64: np.int64,
          BOOL: np.uint8, FLOAT: np.float32, DOUBLE: np.float64}
KINDS = sorted(DTYPES)
C = 256  # gpu/kernels.h kJsonNumberPrintChunkElems


@pytest.fixture(scope="module")
def dev():
    from brpc_amd import native
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert native.gpu.device_count() > 0, "native runtime sees no HIP device"
    assert native.gpu.json_number_print_chunk_elems() == C
    return torch.device("cuda", 0)


def _values(kind, n, seed=0):
    """n elements of `kind`: text lengths from 1 byte to the kind's widest side
    by side (a wrong prefix sum shows up as shifted text), the extremes first."""
    rng = np.random.default_rng(seed * 16 + kind)
    dt = np.dtype(DTYPES[kind])
    if kind == BOOL:
        return rng.choice(np.array([0, 1, 2, 255], dtype=np.uint8), n)
    if kind in (FLOAT, DOUBLE):
        a = rng.standard_normal(n) * np.power(10.0, rng.integers(-30, 30, n))
        a[::5] = np.round(a[::5])
        return a.astype(dt)
    info = np.iinfo(dt)
    bits = rng.integers(0, 1 << 63, n, dtype=np.uint64) >> rng.integers(0, 63, n).astype(np.uint64)
    a = (bits & np.uint64(info.max)).astype(dt)
    if info.min < 0:
        a = np.where(rng.integers(0, 2, n) == 1, a, -a).astype(dt)
    a[:2] = [info.min, info.max][:len(a[:2])]
    return a


def _ragged(n, seed, longest=5):
    rng = np.random.default_rng(seed)
    ends, at = [], 0
    while at < n:
        at = min(n, at + int(rng.integers(1, longest + 1)))
        ends.append(at)
    return ends


def _to_dev(a, dev):
    """The memory image of a numpy array in device memory (uint32 / uint64
    travel as bytes: not every torch has those dtypes)."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)


class Job:
    """One job of a call: source and row ends in device memory and a
    sentinel-filled destination whose text starts at `phase` (mod 16)."""

    def __init__(self, native, dev, a, kind, ends=None, brackets=True, phase=0, cap=None, count=None):
        self.a, self.kind, self.ends, self.brackets = a, kind, ends, brackets
        self.count = len(a) if count is None else count
        self.src = _to_dev(a, dev) if len(a) else None
        self.table = _to_dev(np.asarray(ends, dtype=np.uint32), dev) if ends is not None and len(ends) else None
        self.rows = 0 if ends is None else len(ends)
        self.worst = native.gpu.json_number_print_worst_case(kind, self.count, self.rows)
        self.cap = self.worst if cap is None else cap
        self.buf = torch.full((16 + phase + self.cap + 48,), SENTINEL, dtype=torch.uint8, device=dev)
        self.off = (phase - self.buf.data_ptr()) % 16
        self.twin = native.json_format_number_rows(a.tobytes(), self.count, kind, ends, brackets)

    def args(self):
        return (self.src.data_ptr() if self.src is not None else 0, self.count, self.kind,
                self.table.data_ptr() if self.table is not None else 0, self.rows, self.brackets,
                self.buf.data_ptr() + self.off, self.cap)

    def check(self, result):
        """The device's result against the twin's, and every byte of the buffer."""
        length, first_bad, err = result
        t_err, t_bad, t_text = self.twin
        got = bytes(self.buf.cpu().numpy())
        if t_err == 0 and len(t_text) > self.cap:
            assert (length, first_bad, err) == (len(t_text), NONE, 3)
            t_text = b""
        else:
            assert (err, first_bad) == (t_err, t_bad)
            if err == 0:
                assert length == len(t_text)
        assert got[self.off:self.off + len(t_text)] == t_text
        assert got[:self.off] == bytes([SENTINEL]) * self.off  # nothing before the text
        rest = got[self.off + len(t_text):]
        assert rest == bytes([SENTINEL]) * len(rest)  # and nothing behind it


def _run(native, jobs):
    torch.cuda.synchronize()
    cols = list(zip(*[j.args() for j in jobs]))
    results = native.gpu.device_json_print_numbers(*[list(c) for c in cols], 0)
    assert len(results) == len(jobs)
    for j, r in zip(jobs, results):
        j.check(r)
    return results


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, C - 1, C, C + 1, 3 * C + 1])
def test_counts_every_kind_three_forms(native, dev, kind, n):
    a = _values(kind, n, seed=n)
    jobs = [Job(native, dev, a, kind, None, False), Job(native, dev, a, kind, None, True),
            Job(native, dev, a, kind, _ragged(n, seed=n), False)]
    for r in _run(native, jobs):
        assert r[2] == 0
    assert jobs[2].twin[2].startswith(b"[[") and jobs[1].twin[2] == b"[" + jobs[0].twin[2] + b"]"


def test_long_job_crosses_the_prefix_tile(native, dev):
    n = 300 * C
    a = np.random.default_rng(1).integers(0, 128000, n).astype(np.int32)
    (length, _, err), = _run(native, [Job(native, dev, a, INT32, list(range(32, n + 1, 32)))])
    assert err == 0 and length > n


def test_row_edges(native, dev):
    a = _values(INT64, 3 * C + 7, seed=3)
    n = len(a)
    tables = [
        [C, 2 * C, 3 * C, n],             # rows that end exactly on a chunk edge
        [C - 1, C, C + 1, 2 * C - 1, 2 * C + 1, n],  # and around it
        [10, 10 + 2 * C + 50, n],         # a row that spans three chunks
        [n],                              # one row over all chunks
        [5, n - 1, n],                    # a last row of one element
    ]
    jobs = [Job(native, dev, a, INT64, t) for t in tables]
    for rows in (C + 1, 2 * C + 1):       # rows of one element, a block of rows and one more
        jobs.append(Job(native, dev, a[:rows], INT64, list(range(1, rows + 1))))
    jobs.append(Job(native, dev, _values(FLOAT, 2 * C, seed=4), FLOAT, [C, 2 * C]))
    for r in _run(native, jobs):
        assert r[2] == 0


def test_extremes(native, dev):
    u64 = [0] + [v for k in range(1, 20) for v in (10 ** k - 1, 10 ** k)] + [2 ** 64 - 1]
    i64 = [s * v for k in range(1, 19) for v in (10 ** k - 1, 10 ** k) for s in (1, -1)] + [-2 ** 63, 2 ** 63 - 1]
    i32 = [-2 ** 31, -10 ** 9, -(10 ** 9 - 1), -10, -9, -1, 0, 9, 10, 99, 100, 10 ** 9 - 1, 10 ** 9, 2 ** 31 - 1]
    jobs = [Job(native, dev, np.array(u64, dtype=np.uint64), UINT64),
            Job(native, dev, np.array(i64, dtype=np.int64), INT64, brackets=False),
            Job(native, dev, np.array(i64, dtype=np.int64), SINT64, _ragged(len(i64), 1)),
            Job(native, dev, np.array(i32, dtype=np.int32), INT32),
            Job(native, dev, np.array(i32, dtype=np.int32), SINT32, [1, len(i32)]),
            Job(native, dev, np.array(i32, dtype=np.int32).view(np.uint32), UINT32),
            Job(native, dev, np.array([0, 1, 2, 255], dtype=np.uint8), BOOL, [1, 4]),
            Job(native, dev, np.array([np.nan, np.inf, -np.inf, -0.0, 5e-324, 1.7976931348623157e308]), DOUBLE, [3, 6])]
    for r in _run(native, jobs):
        assert r[2] == 0
    assert jobs[0].twin[2].endswith(b",9999999999999999999,10000000000000000000,18446744073709551615]")
    assert jobs[1].twin[2].endswith(b",-9223372036854775808,9223372036854775807")
    assert jobs[4].twin[2].startswith(b"[[-2147483648],[-1000000000,")
    assert jobs[6].twin[2] == b"[[false],[true,true,true]]"
    assert jobs[7].twin[2].startswith(b'[["NaN","Infinity","-Infinity"],[-0.0,5e-324,')


@pytest.mark.parametrize("phase", [0, 1, 15])
def test_alignment_of_dst(native, dev, phase):
    """Job.check compares every byte before and behind the text with the sentinel."""
    a = _values(INT32, 2 * C + 9, seed=5)
    jobs = [Job(native, dev, a, INT32, _ragged(len(a), 2), phase=phase),
            Job(native, dev, a[:5], INT32, None, False, phase=phase),
            Job(native, dev, _values(DOUBLE, C + 3, seed=6), DOUBLE, None, True, phase=phase)]
    for r in _run(native, jobs):
        assert r[2] == 0


def test_capacity(native, dev):
    a = _values(INT64, 2 * C + 1, seed=7)
    ends = _ragged(len(a), 3)
    need = len(native.json_format_number_rows(a.tobytes(), len(a), INT64, ends, True)[2])
    exact, short = Job(native, dev, a, INT64, ends, cap=need), Job(native, dev, a, INT64, ends, cap=need - 1)
    none = Job(native, dev, a, INT64, ends, cap=0)
    results = _run(native, [exact, short, none])  # check(): dst all sentinel where the text does not fit
    assert results == [(need, NONE, 0), (need, NONE, 3), (need, NONE, 3)]
    assert native.gpu.json_number_print_worst_case(INT64, len(a), len(ends)) >= need


def test_bad_row_ends(native, dev):
    a = _values(INT32, 10, seed=8)
    cases = [([3, 2, 10], 1),   # a decrease
             ([3, 3, 10], 1),   # two equal neighbours
             ([0, 5, 10], 0),   # row_ends[0] == 0
             ([3, 11, 12], 1),  # an end above count
             ([3, 5, 9], 2),    # a last end below count
             ([3, 5, 4, 4, 10], 2),      # the lowest of several
             ([0xFFFFFFFF, 10], 0)]
    jobs = [Job(native, dev, a, INT32, ends) for ends, _ in cases]
    # bad rows far along: in the second block of rows, and the last row of the third
    big = _values(INT32, 3 * C, seed=9)
    ones = list(range(1, 3 * C + 1))
    late = ones[:C + 7] + [ones[C + 6]] + ones[C + 8:]
    jobs += [Job(native, dev, big, INT32, late), Job(native, dev, big, INT32, ones[:-1] + [3 * C + 1]),
             Job(native, dev, big, INT32, ones, count=3 * C - 1)]
    good = Job(native, dev, a, INT32, [3, 5, 10])
    results = _run(native, jobs[:4] + [good] + jobs[4:])  # check(): dst untouched unless printed
    assert results.pop(4) == (len(good.twin[2]), NONE, 0)
    want = [bad for _, bad in cases] + [C + 7, 3 * C - 1, 3 * C - 1]
    assert [(r[1], r[2]) for r in results] == [(bad, 1) for bad in want]
    # rows over no elements
    empty = Job(native, dev, np.zeros(0, dtype=np.int32), INT32, [1])
    assert _run(native, [empty, good]) == [(0, 0, 1), (len(good.twin[2]), NONE, 0)]


def test_refusals(native, dev):
    src = torch.zeros(64, dtype=torch.int64, device=dev)
    ends = torch.tensor([4], dtype=torch.int32, device=dev)
    dst = torch.full((256,), SENTINEL, dtype=torch.uint8, device=dev)
    s, e, d = src.data_ptr(), ends.data_ptr(), dst.data_ptr()
    torch.cuda.synchronize()

    def code(src, count, kind, row_ends, rows, brackets, dst, cap):
        (length, first_bad, err), = native.gpu.device_json_print_numbers([src], [count], [kind], [row_ends], [rows],
                                                                         [brackets], [dst], [cap], 0)
        assert (length, first_bad) == (0, NONE)
        return err

    assert code(0, 0, INT32, 0, 0, False, 0, 0) == 0          # bare and empty: nothing written, nothing launched
    assert code(s, 4, 7, 0, 0, True, d, 256) == 2             # kind 7
    assert code(s, 4, 10, 0, 0, True, d, 256) == 2            # above 9
    assert code(0, 4, INT32, 0, 0, True, d, 256) == 2         # null src
    assert code(s, 4, INT32, 0, 0, True, 0, 256) == 2         # null dst
    assert code(0, 0, INT32, 0, 0, True, 0, 256) == 2         # "[]" has to go somewhere
    assert code(s + 2, 4, INT32, 0, 0, True, d, 256) == 2     # an int32 at 2 (mod 4)
    assert code(s + 4, 4, INT64, 0, 0, True, d, 256) == 2     # an int64 at 4 (mod 8)
    assert code(s + 4, 4, DOUBLE, 0, 0, True, d, 256) == 2    # a double at 4 (mod 8)
    assert code(s + 2, 4, FLOAT, 0, 0, True, d, 256) == 2     # a float at 2 (mod 4)
    assert code(s, 4, INT32, s + 66, 1, True, d, 256) == 2    # row_ends at 2 (mod 4)
    assert code(s, 4, INT32, 0, 1, True, d, 256) == 2         # rows without row_ends
    assert code(s, 4, INT32, e, 0, True, d, 256) == 2         # row_ends without rows
    assert code(s, 4, INT32, 0, 0, True, s + 15, 64) == 2     # dst overlaps src
    assert code(s + 32, 4, INT32, 0, 0, True, s, 33) == 2     # dst runs into src
    assert code(s, 4, INT32, s + 64, 1, True, s + 60, 64) == 2  # dst overlaps row_ends
    assert code(s, 1 << 32, BOOL, 0, 0, True, d, 256) == 2    # a worst case above 2^32 - 1
    assert code(s, 4, INT32, e, 1 << 31, True, d, 256) == 2   # by its rows alone
    assert bytes(dst.cpu().numpy()) == bytes([SENTINEL]) * 256
    assert not src.any()
    # a refused job beside a good one
    a = _values(INT32, 9, seed=1)
    good = Job(native, dev, a, INT32)
    torch.cuda.synchronize()
    res = native.gpu.device_json_print_numbers([s, good.args()[0]], [4, 9], [7, INT32], [0, 0], [0, 0], [True, True],
                                               [d, good.args()[6]], [256, good.cap], 0)
    assert res[0] == (0, NONE, 2)
    good.check(res[1])
    assert native.gpu.json_number_print_worst_case(7, 3) == 0
    assert native.gpu.json_number_print_worst_case(INT32, 3) == 3 * 11 + 4
    assert native.gpu.json_number_print_worst_case(DOUBLE, 3, 2) == 3 * 25 + 3 + 5


def test_mixed_jobs_in_one_call(native, dev):
    jobs = [Job(native, dev, _values(INT32, 2 * C + 3, 1), INT32, _ragged(2 * C + 3, 1), phase=3),
            Job(native, dev, _values(DOUBLE, C, 2), DOUBLE, None, False, phase=9),
            Job(native, dev, np.zeros(0, dtype=np.int64), INT64, None, True),   # "[]"
            Job(native, dev, _values(BOOL, C + 1, 3), BOOL, _ragged(C + 1, 2, longest=40)),
            Job(native, dev, np.zeros(0, dtype=np.float32), FLOAT, None, False),  # nothing
            Job(native, dev, _values(UINT64, 77, 4), UINT64, [77], phase=15),
            Job(native, dev, _values(FLOAT, 3 * C, 5), FLOAT, [1, 2, 3 * C], cap=40),  # too long for its cap
            Job(native, dev, _values(SINT32, 5, 6), SINT32, [2, 2, 5]),           # bad rows
            Job(native, dev, _values(INT64, 1, 7), INT64, [1])]
    results = _run(native, jobs)
    assert [r[2] for r in results] == [0, 0, 0, 0, 0, 0, 3, 1, 0]
    assert results[2][0] == 2 and results[4][0] == 0 and results[7][1] == 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_flat_floats_equal_json_print_floats(native, dev, dtype):
    from brpc_amd import ops
    t = torch.from_numpy(_values(DOUBLE, 2 * C + 5, seed=11)).to(dev).to(dtype)
    t[3], t[4] = float("nan"), float("-inf")
    flat = ops.json_print_numbers(t, brackets=False)
    assert torch.equal(flat, ops.json_print_floats(t))
    assert bytes(ops.json_print_numbers(t).cpu().numpy()) == b"[" + bytes(flat.cpu().numpy()) + b"]"


def test_ops_forms_and_dtypes(native, dev):
    from brpc_amd import ops
    text = lambda *a, **k: bytes(ops.json_print_numbers(*a, **k).cpu().numpy())  # noqa: E731
    ids = torch.tensor([[1, -2, 3], [40, 50, -60]], device=dev)
    assert text(ids) == b"[[1,-2,3],[40,50,-60]]"                       # 2-D: equal rows
    assert text(ids.to(torch.int32).t()) == b"[[1,40],[-2,50],[3,-60]]"   # not contiguous
    assert text(ids.view(-1)) == b"[1,-2,3,40,50,-60]"
    assert text(ids.view(-1), brackets=False) == b"1,-2,3,40,50,-60"
    ends = torch.tensor([1, 6], device=dev)
    assert text(ids, ends) == b"[[1],[-2,3,40,50,-60]]"                 # row_ends over the flattened values
    assert text(ids.view(-1), ends.to(torch.int32), brackets=False) == b"[[1],[-2,3,40,50,-60]]"
    assert text(ids.view(-1) > 0, ends) == b"[[true],[false,true,true,true,false]]"
    assert text(torch.tensor([0.5, 2.0], device=dev), torch.tensor([2], device=dev)) == b"[[0.5,2.0]]"
    if hasattr(torch, "uint64"):
        big = torch.tensor([2 ** 63 - 1], device=dev).view(torch.uint64)
        assert text(big) == b"[9223372036854775807]"
    for dt in (torch.int32, torch.int64, torch.bool, torch.float32, torch.float64):
        none = torch.empty(0, dtype=dt, device=dev)
        assert text(none) == b"[]" and text(none, brackets=False) == b""
        assert text(none.view(0, 0)) == b"[]"
        assert text(none, torch.empty(0, dtype=torch.int64, device=dev)) == b"[]"
    with pytest.raises(ValueError, match=r"row_ends\[1\]"):
        ops.json_print_numbers(ids, torch.tensor([3, 3, 6], device=dev))
    with pytest.raises(ValueError, match=r"row_ends\[0\]"):
        ops.json_print_numbers(ids, torch.tensor([-1, 6], device=dev))
    with pytest.raises(ValueError, match=r"row_ends\[1\]"):
        ops.json_print_numbers(ids, torch.tensor([3, 1 << 40], device=dev))
    with pytest.raises(ValueError):
        ops.json_print_numbers(ids, torch.empty(0, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        ops.json_print_numbers(torch.empty((3, 0), device=dev))
    with pytest.raises(TypeError):
        ops.json_print_numbers(ids.to(torch.int16))
    with pytest.raises(TypeError):
        ops.json_print_numbers(ids, [3, 6])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_round_trip_floats(native, dev, dtype):
    from brpc_amd import ops
    n = 3 * C + 11
    t = torch.from_numpy(_values(DOUBLE, n, seed=12)).to(dev).to(dtype)
    ends = torch.tensor(_ragged(n, 5, longest=300), device=dev)
    text = ops.json_print_numbers(t, ends)
    values, row_ends = ops.json_parse_float_rows(text, dtype, ragged=True)
    assert torch.equal(values.view(torch.int32 if dtype == torch.float32 else torch.int64),
                       t.view(torch.int32 if dtype == torch.float32 else torch.int64))  # bit for bit
    assert torch.equal(row_ends, ends)
    assert torch.equal(ops.json_print_numbers(values, row_ends), text)  # taken back unchanged
    square = t[:3 * C].view(12, -1)
    assert torch.equal(ops.json_parse_float_rows(ops.json_print_numbers(square), dtype), square)
    assert torch.equal(ops.json_parse_floats(ops.json_print_numbers(t), dtype), t)


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_round_trip_ints(native, dev, dtype):
    from brpc_amd import ops
    n = 2 * C + 5
    t = torch.from_numpy(_values(INT32 if dtype == torch.int32 else INT64, n, seed=13)).to(dev)
    ends = torch.tensor(_ragged(n, 6, longest=70), device=dev)
    text = ops.json_print_numbers(t, ends)
    values, row_ends = ops.json_parse_int_rows(text, dtype, ragged=True)
    assert values.dtype == dtype and torch.equal(values, t) and torch.equal(row_ends, ends)
    square = t[:2 * C].view(8, -1)
    assert torch.equal(ops.json_parse_int_rows(ops.json_print_numbers(square), dtype), square)
    assert torch.equal(ops.json_parse_ints(ops.json_print_numbers(t), dtype), t)
    assert torch.equal(ops.json_parse_ints(ops.json_print_numbers(t, brackets=False), dtype), t)
    assert ops.json_parse_int_rows(torch.tensor(list(b"[ ]"), dtype=torch.uint8, device=dev), dtype).shape == (0, 0)
    assert ops.json_parse_ints(torch.empty(0, dtype=torch.uint8, device=dev), dtype).numel() == 0


def test_json_parse_ints_refusals(native, dev):
    from brpc_amd import ops
    text = lambda s: torch.tensor(list(s), dtype=torch.uint8, device=dev)  # noqa: E731
    assert ops.json_parse_ints(text(b"[1, -2,3]")).tolist() == [1, -2, 3]
    assert ops.json_parse_ints(text(b"9223372036854775807,-9223372036854775808")).tolist() == [2 ** 63 - 1, -2 ** 63]
    assert ops.json_parse_ints(text(b"2147483647,-2147483648"), torch.int32).tolist() == [2 ** 31 - 1, -2 ** 31]
    with pytest.raises(ValueError, match="element 2 is not an integer"):
        ops.json_parse_ints(text(b"[1,2,1.5,9223372036854775808]"))
    with pytest.raises(ValueError, match="element 1 is above INT64_MAX"):
        ops.json_parse_ints(text(b"[1,9223372036854775808,1.5]"))
    with pytest.raises(ValueError, match="element 3 does not fit int32"):
        ops.json_parse_ints(text(b"0,1,2,2147483648,1.5"), torch.int32)
    with pytest.raises(ValueError, match="element 0 does not fit int32"):
        ops.json_parse_ints(text(b"-2147483649,5"), torch.int32)
    # 25 digits, halfway between two doubles: no 19-digit truncation decides it, so it comes back on the redo list
    long_int = str(2 ** 80 + 2 ** 27).encode()
    assert len(long_int) == 25 and native.json_parse_numbers(long_int, False)[1][0] == 3
    longer = b"1" + b"0" * native.json_max_device_number_chars()  # too long for a lane
    with pytest.raises(ValueError, match="element 2 is not an integer"):
        ops.json_parse_ints(text(b"7,8," + longer + b"," + long_int))
    with pytest.raises(ValueError, match="element 1 is not an integer"):
        ops.json_parse_ints(text(b"[7," + long_int + b",1.5]"))
    with pytest.raises(ValueError, match="element 1 is not an integer"):
        ops.json_parse_int_rows(text(b"[[7," + long_int + b"],[" + long_int + b"]]"))
    with pytest.raises(ValueError, match="element 0 is not an integer"):
        ops.json_parse_ints(text(b"1e3,1.5"))
    with pytest.raises(ValueError, match="element 1 is not a JSON number"):
        ops.json_parse_ints(text(b"1,x"))
    with pytest.raises(TypeError):
        ops.json_parse_ints(text(b"1"), torch.float32)
    with pytest.raises(TypeError):
        ops.json_parse_floats(text(b"1"), torch.int64)
