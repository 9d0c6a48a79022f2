"""pb::SplitRows (native.pb_split_rows), the host twin of the device row
splitter, against this directory's pure-python splitter
(pb_rows_split_ref.split) on every message the GPU tests run, and as the
inverse of pb::SerializeRows. pb_rows::SpecField's two invariants run in
brpc_amd/csrc/tests/pb_rows_split_unittest.cc."""
import pytest

np = pytest.importorskip("numpy")

import pb_rows_split_ref as R  # noqa: E402
import pb_rows_wire as W  # noqa: E402


@pytest.fixture(scope="module")
def native():
    from brpc_amd import native
    return native


def _same(native, number, inner, kind, msg, **caps):
    want = R.split(number, inner, kind, msg, caps.get("cap"), caps.get("row_cap"))
    got = native.pb_split_rows(number, inner, kind, bytes(msg), caps.get("cap"), caps.get("row_cap"))
    assert tuple(got) == want
    return want


@pytest.mark.parametrize("kind,inner", R.ALL)
def test_chunk_seams_and_the_way_back(native, kind, inner):
    msg, arr = R.boundary_message(kind, inner)
    err, count, rows, others, _, values, ends = _same(native, 4, inner, kind, msg)
    assert (err, count, rows, others) == (0, arr.size, R.BOUNDARY_ENDS.size, 0)
    assert ends == [int(e) for e in R.BOUNDARY_ENDS]
    # bools come back as 0 / 1, everything else as it was
    assert values == ((arr != 0).astype(np.uint8) if kind == 6 else arr).tobytes()
    # SerializeRows(SplitRows(m)) == m
    assert native.pb_serialize_rows(4, inner, kind, values, ends)[2] == msg


@pytest.mark.parametrize("kind,inner", [(1, 2), (W.FIXED32, 2), (W.BYTES, 0)])
def test_a_foreign_field_of_every_length_in_front(native, kind, inner):
    msg, arr = R.boundary_message(kind, inner)
    for length in range(41):
        err, count, _, others, _, _, _ = _same(native, 4, inner, kind, R.bytes_field(9, b"\x22" * length) + msg)
        assert (err, count, others) == (0, arr.size, 1)


def test_payload_that_looks_like_wire(native):
    for kind, inner, msg in R.wire_like_cases():
        assert _same(native, 4, inner, kind, msg)[0] == 0


def test_field_numbers(native):
    for number in R.NUMBERS:
        for inner in R.NUMBERS:
            msg, arr = R.small_message(2, inner, number=number)
            assert _same(native, number, inner, 2, msg)[:2] == (0, arr.size)


def test_foreign_fields_are_counted(native):
    for kind, inner, msg, others in R.foreign_cases():
        got = _same(native, 4, inner, kind, msg)
        assert got[0] == 0 and got[2] == 4 and got[3] == others


def test_noncanonical_varints_are_accepted(native):
    for kind, inner, msg in R.noncanonical_cases():
        err, count, rows, others, _, values, ends = _same(native, 4, inner, kind, msg)
        assert (err, count, rows, others, ends) == (0, 6, 3, 1, [3, 6, 6])
        assert values == np.array([1, 300, 70000] * 2, dtype=np.uint32).tobytes()


def test_malformed(native):
    for kind, inner, msg in R.malformed_cases():
        got = _same(native, 4, inner, kind, msg)
        assert got[0] == 1 and got[4] < len(msg) and got[5] == b"" and got[6] == []
    codes = [_same(native, 4, inner, kind, msg)[0] for kind, inner, msg in R.cut_cases()]
    assert set(codes) == {0, 1} and codes.count(1) >= 18


def test_unsupported_shapes(native):
    for kind, inner, msg, code in R.unsupported_cases():
        assert _same(native, 4, inner, kind, msg)[0] == code


def test_capacities(native):
    msg, arr = R.small_message(1, 2)
    rows = 6
    assert _same(native, 4, 2, 1, msg, cap=arr.size, row_cap=rows)[0] == 0
    assert _same(native, 4, 2, 1, msg, cap=arr.size - 1, row_cap=rows)[:3] == (5, arr.size, rows)
    assert _same(native, 4, 2, 1, msg, cap=arr.size, row_cap=rows - 1)[:3] == (5, arr.size, rows)


def test_refusals_and_the_empty_message(native):
    msg, _ = R.small_message(1, 2)
    for number, inner, kind in [(0, 2, 1), (2**29, 2, 1), (4, 2**29, 1), (4, 0, 1)]:
        assert _same(native, number, inner, kind, msg)[0] == 2
    with pytest.raises(ValueError):
        native.pb_split_rows(4, 2, 10, msg)
    assert _same(native, 4, 2, 1, b"")[:4] == (0, 0, 0, 0)


@pytest.mark.parametrize("kind,inner", R.ALL)
def test_the_host_serializer_s_bytes_split_to_the_same_arrays(native, tmp_path, kind, inner):
    sizes = [0, 3, 0, 0, 2045, 1, 2, 700, 0, 64, 63, 65, 0]
    arr = W.values(kind, sum(sizes), 200 + kind)
    wire, _, _ = W.host_wire(native, tmp_path, kind, 4, inner, arr, np.cumsum(sizes))
    err, count, rows, _, _, values, ends = _same(native, 4, inner, kind, wire)
    assert err == 0 and ends == [int(e) for e in np.cumsum(sizes)]
    assert values == ((arr != 0).astype(np.uint8) if kind == 6 else arr).tobytes()
