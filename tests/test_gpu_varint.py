"""Packed-varint codec (gpu/kernels.hip varint_count / varint_decode /
varint_len / varint_encode kernels and the scan_tiles_kernel between them)
where the small round trips of test_gpu_ops.py do not reach: more than 1024
tiles, so every lane of the scan owns more than one tile; zigzag at full
width; input that is not 16-byte aligned; a 10-byte varint laid across the
16-byte lane, 1 KiB wave and 4 KiB tile seams at each of its 9 split points;
and the output capacity check.

The reference is this file's vectorised numpy encoder, pinned without a GPU to
the pure-python varint_encode_host. Bytes and values are compared exactly."""
import pytest

torch = pytest.importorskip("torch")
np = pytest.importorskip("numpy")

TILE = 4096  # bytes (decode) or values (encode) per workgroup: kVTile


def _np_varints(wire):
    """Vectorised protobuf varint encoding of a uint64 array -> uint8 array."""
    wire = np.ascontiguousarray(wire, dtype=np.uint64)
    nbytes = np.ones(wire.shape, dtype=np.int64)
    for k in range(1, 10):
        nbytes += (wire >> np.uint64(7 * k)) > 0
    start = np.cumsum(nbytes) - nbytes
    out = np.zeros(int(nbytes.sum()), dtype=np.uint8)
    for k in range(10):
        m = nbytes > k
        byte = ((wire[m] >> np.uint64(7 * k)) & np.uint64(0x7F)).astype(np.uint8)
        byte |= np.where(nbytes[m] > k + 1, 0x80, 0).astype(np.uint8)
        out[start[m] + k] = byte
    return out, nbytes


def _np_zigzag(v):
    v = np.ascontiguousarray(v, dtype=np.int64)
    return ((v << 1) ^ (v >> 63)).view(np.uint64)


def _mixed(n, seed):
    """uint64 values of every encoded length 1..10, evenly mixed."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 2**64, n, dtype=np.uint64) >> rng.integers(0, 64, n).astype(np.uint64)


def test_numpy_reference_matches_host_encoder():
    from brpc_amd.ops import varint_decode_host, varint_encode_host
    vals = np.concatenate([np.array([0, 1, 127, 128, 16383, 16384, 2**63 - 1, 2**63, 2**64 - 1], dtype=np.uint64),
                           _mixed(1991, 1)])
    assert len(vals) == 2000
    enc, nbytes = _np_varints(vals)
    assert sorted(set(nbytes.tolist())) == list(range(1, 11))
    signed = vals.view(np.int64).tolist()
    assert enc.tobytes() == varint_encode_host(signed)
    assert varint_decode_host(enc.tobytes()) == signed
    zz, _ = _np_varints(_np_zigzag(vals.view(np.int64)))
    assert zz.tobytes() == varint_encode_host(signed, zigzag=True)


@pytest.fixture(scope="module")
def dev():
    from brpc_amd import native
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert native.gpu.device_count() > 0, "native runtime sees no HIP device"
    assert native.gpu.device_arch(0) == "gfx950"
    return torch.device("cuda", 0)


def _dev_i64(u64, dev):
    return torch.from_numpy(np.ascontiguousarray(u64).view(np.int64)).to(dev)


@pytest.mark.gpu
def test_varint_decode_more_tiles_than_scan_lanes(dev):
    """4 MiB + 1000 bytes are 1025 tiles: scan_tiles_kernel's lanes own 2
    tiles each (per == 2), and every tile's output offset depends on it."""
    from brpc_amd.ops import varint_decode
    target = 4 * (1 << 20) + 1000
    vals = _mixed(1000000, 2)
    enc, nbytes = _np_varints(vals)
    ends = np.cumsum(nbytes)
    k = int(np.searchsorted(ends, target, side="right"))  # values that fit whole
    assert 0 < k < len(vals)
    pad = target - int(ends[k - 1])
    want = np.concatenate([vals[:k], np.arange(pad, dtype=np.uint64) % np.uint64(128)])
    stream = np.concatenate([enc[:int(ends[k - 1])], want[k:].astype(np.uint8)])
    assert len(stream) == target and -(-target // TILE) == 1025
    got = varint_decode(torch.from_numpy(stream).to(dev))
    assert torch.equal(got, _dev_i64(want, dev))


@pytest.mark.gpu
def test_varint_encode_more_tiles_than_scan_lanes(dev):
    """4096 * 1024 + 1 values are 1025 tiles of the encoder: the scan's per
    == 2 decides where every tile's bytes go."""
    from brpc_amd.ops import varint_decode, varint_encode
    n = TILE * 1024 + 1
    vals = _mixed(n, 3)
    want, _ = _np_varints(vals)
    t = _dev_i64(vals, dev)
    enc = varint_encode(t)
    assert enc.numel() == len(want)
    assert torch.equal(enc, torch.from_numpy(want).to(dev))
    assert torch.equal(varint_decode(enc), t)


@pytest.mark.gpu
def test_varint_zigzag_full_width(dev):
    from brpc_amd.ops import varint_decode, varint_encode, varint_encode_host
    rng = np.random.default_rng(4)
    vals = np.concatenate([np.array([-2**63, 2**63 - 1, -1, 0, 1], dtype=np.int64),
                           rng.integers(-2**63, 2**63, 1000, dtype=np.int64)])
    want, _ = _np_varints(_np_zigzag(vals))
    assert want.tobytes() == varint_encode_host(vals.tolist(), zigzag=True)
    t = torch.from_numpy(vals).to(dev)
    enc = varint_encode(t, zigzag=True)
    assert enc.cpu().numpy().tobytes() == want.tobytes()
    assert torch.equal(varint_decode(enc, zigzag=True), t)


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [1, 3])
def test_varint_decode_misaligned_input(dev, shift):
    """The stream starts `shift` bytes into an allocation: the count and
    decode kernels take their byte-wise loads, on three tiles and a tail."""
    from brpc_amd.ops import varint_decode
    vals = _mixed(3000, 5 + shift)
    enc, _ = _np_varints(vals)
    assert len(enc) > 3 * TILE
    buf = torch.from_numpy(np.concatenate([np.full(shift, 0x80, dtype=np.uint8), enc])).to(dev)
    view = buf[shift:]
    assert view.data_ptr() % 16 == shift
    assert torch.equal(varint_decode(view), _dev_i64(vals, dev))


@pytest.mark.gpu
def test_varint_ten_bytes_across_every_seam(dev):
    """A 10-byte varint with k bytes before the seam S, for the 16-byte lane
    seam (the neighbour lane's bytes), the 1 KiB wave seam (lane 0 reloads
    the previous 16 bytes) and the 4 KiB tile seam (another workgroup), k in
    1..9; 20 values of every length follow it."""
    from brpc_amd.ops import varint_decode
    streams, wants, pos = [], [], 0
    pieces = []
    for S in (16, 1024, 4096):
        for k in range(1, 10):
            head = (np.arange(S - k, dtype=np.uint64) * np.uint64(7) + np.uint64(k)) % np.uint64(128)
            big = np.array([(1 << 63) | (0x123456789ABCDEF * (S + k)) % (1 << 63)], dtype=np.uint64)
            want = np.concatenate([head, big, _mixed(20, 100 * S + k)])
            enc, nbytes = _np_varints(want)
            assert nbytes[S - k] == 10 and int(nbytes[:S - k].sum()) == S - k
            pad = -len(enc) % 16  # every stream starts 16-byte aligned
            pieces.append(np.concatenate([enc, np.full(pad, 0x80, dtype=np.uint8)]))
            streams.append((pos, len(enc)))
            wants.append(want)
            pos += len(enc) + pad
    assert len(streams) == 27
    buf = torch.from_numpy(np.concatenate(pieces)).to(dev)
    for (p, n), want in zip(streams, wants):
        got = varint_decode(buf[p:p + n])
        assert got.cpu().numpy().view(np.uint64).tolist() == want.tolist(), (p, n)


@pytest.mark.gpu
def test_varint_decode_capacity(dev):
    from brpc_amd.ops import varint_decode
    vals = _mixed(5000, 8)
    enc, _ = _np_varints(vals)
    buf = torch.from_numpy(enc).to(dev)
    assert torch.equal(varint_decode(buf, max_values=len(vals)), _dev_i64(vals, dev))
    with pytest.raises(ValueError):
        varint_decode(buf, max_values=len(vals) - 1)
