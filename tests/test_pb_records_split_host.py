"""pb::SplitRecords (native.pb_split_records), the host twin of the device
record splitter, against this directory's pure-python splitter
(pb_records_split_ref.split) on every message the GPU tests run, and as the
inverse of pb::SerializeRecords. pb_records::RecordShape's rules run one by
one in brpc_amd/csrc/tests/pb_records_split_unittest.cc."""
import pytest

np = pytest.importorskip("numpy")

import pb_records_split_ref as S  # noqa: E402
import pb_records_wire as RW  # noqa: E402


@pytest.fixture(scope="module")
def native():
    from brpc_amd import native
    return native


def _same(native, job):
    want = S.split(job["number"], job["cols"], job["msg"], job.get("row_cap"), job.get("caps"))
    got = native.pb_split_records(job["number"], job["cols"], bytes(job["msg"]), job.get("row_cap"), job.get("caps"))
    assert (got[0], got[1], got[2], got[3], [tuple(c) for c in got[4]]) == want
    assert want[0] in (0, 1, 2, 5, 6)
    return want


def _as_expected(job, got):
    """What the case itself says of its result."""
    err, rows, others, first_bad, cols = got
    assert err == job.get("code", 0)
    if "first_bad" in job:
        assert first_bad == job["first_bad"]
    if err in (0, 5) and "rows" in job:
        assert rows == job["rows"]
    if err == 0:
        assert others == job.get("others", 0)
        if "values" in job:
            assert [(c[2], c[3]) for c in cols] == job["values"]
        assert [c[1] for c in cols] == job.get("absent", [0] * len(cols))
    if "counts" in job:
        assert [c[0] for c in cols] == job["counts"]


def test_every_case_of_the_gpu_file(native):
    for job in S.all_cases():
        _as_expected(job, _same(native, job))


def test_serialize_records_gives_the_bytes_back(native):
    """SerializeRecords(SplitRecords(m)) == m for canonical builder output."""
    for job in S.round_trip_cases() + S.record_count_cases() + S.element_count_cases():
        _, rows, _, _, cols = _same(native, job)
        back = native.pb_serialize_records(
            job["number"], [(inner, kind, c[2], c[3]) for (inner, kind, _), c in zip(job["cols"], cols)], rows)
        assert back[0] == 0 and back[3] == job["msg"]


def test_truncations(native):
    """The seam message cut at each of its last 24 lengths: code 1 at the
    record that is cut, or a shorter whole message."""
    columns, msg = S.seam_message()
    codes = []
    for k in range(1, 25):
        got = _same(native, dict(number=4, cols=S.split_columns(columns), msg=msg[:len(msg) - k]))
        codes.append(got[0])
        assert got[0] == 0 or got[3] < len(msg) - k
    assert set(codes) <= {0, 1} and codes.count(1) >= 12


def test_refusals_and_the_empty_message(native):
    msg = S.good_example()
    for number, cols in S.refused_cases():
        assert _same(native, dict(number=number, cols=cols, msg=msg))[0] == 2
    got = _same(native, dict(number=4, cols=S.EXAMPLE_COLS, msg=b""))
    assert got[:3] == (0, 0, 0) and [c[0] for c in got[4]] == [0, 0, 0, 0]
    with pytest.raises(ValueError):
        native.pb_split_records(4, S.EXAMPLE_COLS, msg, None, [1, 2])


def test_the_host_serializer_s_bytes_split_to_the_same_columns(native, tmp_path):
    columns = S.make_columns(S.EXAMPLE, 20, 13, 4)
    wire, _, _ = RW.host_wire(native, tmp_path, 4, columns, 20)
    got = _same(native, dict(number=4, cols=S.split_columns(columns), msg=wire))
    assert got[0] == 0 and [(c[2], c[3]) for c in got[4]] == S.expected(columns)
