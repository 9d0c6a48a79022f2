// Batched protobuf wire scan on CDNA4 (gfx950): the device half of the pb
// "unpack" (SURVEY K1 — the per-message tag/varint walk of
// ParsePbFromIOBuf, protocol.h:207, and of RpcMeta at
// baidu_rpc_protocol.cpp:323,563). Many small messages (RpcMeta-sized,
// 20-200 bytes) are packed back to back in HBM with an int64 offset table;
// one launch decodes every top-level field of every message into a
// fixed-width table:
//   fields[i][k] = { (field_number << 3) | wire_type, value }
// where value is the varint (wire 0), the little-endian fixed64/fixed32
// (wires 1/5), or (offset_in_message << 32) | length for length-delimited
// fields (wire 2), which a second pass (or the host) can descend into.
// nfields[i] = number of fields, or a negative code: -1 truncated/malformed,
// -2 more than max_fields fields, -3 field number 0, -4 unsupported wire
// type (proto2 groups), -5 offsets outside the buffer or descending (the
// message is not read at all).
//
// Layout: one lane per message. Messages are tiny and independent, so the
// serial tag walk of one message costs one lane, not one wave; a lane reads
// its message sequentially (the 128-byte lines it touches stay in L1 while
// the lane walks them) and writes its field rows with 16-byte stores.
#include <hip/hip_runtime.h>

#include "base/pb_records.h"
#include "base/pb_rows.h"
#include "gpu/kernels.h"
#include "gpu/device_pb.h"
#include "gpu/workgroup.h"

namespace mrpc {
namespace gpu {

namespace {

typedef const __attribute__((address_space(1))) uint8_t gbyte_c;
using wg::u32x4;

__global__ void __launch_bounds__(256) pb_scan_kernel(const uint8_t* __restrict__ buf_,
                                                      uint64_t buf_len, const int64_t* __restrict__ offsets,
                                                      int64_t n, uint32_t max_fields, uint64_t* __restrict__ fields,
                                                      int32_t* __restrict__ nfields) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    gbyte_c* b = (gbyte_c*)buf_;
    const int64_t so = offsets[i], eo = offsets[i + 1];
    // never trust the offset table: a message must lie inside the buffer
    if (so < 0 || eo < so || (uint64_t)eo > buf_len) {
        nfields[i] = -5;
        return;
    }
    const uint64_t start = (uint64_t)so;
    const uint64_t end = (uint64_t)eo;
    nfields[i] = devpb::scan_message(b, start, end, fields + (uint64_t)i * max_fields * 2, max_fields);
}

// Messages in separate buffers (one per job): the batched codec path, where
// every request decoded its body into its own HBM block.
__global__ void __launch_bounds__(256) pb_scan_ptrs_kernel(const PbScanJob* __restrict__ jobs, int64_t n,
                                                           uint32_t max_fields, uint64_t* __restrict__ fields,
                                                           int32_t* __restrict__ nfields) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PbScanJob job = jobs[i];
    nfields[i] = devpb::scan_message((gbyte_c*)job.buf, 0, job.len, fields + (uint64_t)i * max_fields * 2, max_fields);
}

// ------------------------------------------------------------ run encoder
// The device half of body encode (the reference serializes every
// body on the host: SerializeAsCompressedData, src/brpc/compress.cpp:92,
// called from baidu_rpc_protocol.cpp's response path) and of pb2json's
// number printing (src/json2pb/pb_to_json.cpp, K6).
// One workgroup (4 waves) per PbRunChunk. The chunk is walked in 8 rounds
// of 256 consecutive elements: lane t of round r takes element 256r + t
// (a coalesced 1/4/8-byte load from the source, pinned host or HBM), the
// encoded lengths are block-scanned and every lane writes its bytes into the
// chunk's output image in LDS (<= 21 B per element: 43 KiB). The image then
// leaves through wg::copy_out_bytes, 16-byte stores for the aligned middle:
// over PCIe to pinned host memory a wave's byte stores make 64-byte writes,
// its 16-byte stores 1 KiB ones.
constexpr int kRunThreads = 256;
constexpr uint32_t kRunMaxElemBytes = 21;  // "-9223372036854775808" + ','

// Raw element bits: signed 32-bit kinds sign-extended, bools as 0/1.
__device__ __forceinline__ uint64_t run_load(const void* src, uint32_t i, uint32_t kind) {
    switch (kind) {
    case PB_RUN_INT32:
    case PB_RUN_SINT32: return (uint64_t)(int64_t)static_cast<const int32_t*>(src)[i];
    case PB_RUN_UINT32: return static_cast<const uint32_t*>(src)[i];
    case PB_RUN_BOOL: return static_cast<const uint8_t*>(src)[i] ? 1 : 0;
    default: return static_cast<const uint64_t*>(src)[i];
    }
}

// Wire value of an element (zigzag for sint kinds).
__device__ __forceinline__ uint64_t run_value(uint64_t raw, uint32_t kind) {
    switch (kind) {
    case PB_RUN_SINT32: {
        const int32_t v = (int32_t)raw;
        return (uint32_t)(((uint32_t)v << 1) ^ (uint32_t)(v >> 31));
    }
    case PB_RUN_SINT64: return (raw << 1) ^ (uint64_t)((int64_t)raw >> 63);
    default: return raw;
    }
}

// For decimal output the value is printed as its field type says: signed
// kinds as two's complement of their width (zigzag undone: the JSON shows
// the number, not its wire form).
__device__ __forceinline__ bool run_negative(uint64_t raw, uint32_t kind, uint64_t* mag) {
    const bool is_signed = kind == PB_RUN_INT32 || kind == PB_RUN_SINT32 || kind == PB_RUN_INT64 ||
                           kind == PB_RUN_SINT64;
    const bool neg = is_signed && (int64_t)raw < 0;
    *mag = neg ? (uint64_t)0 - raw : raw;
    return neg;
}

__device__ __forceinline__ uint32_t run_varint_len(uint64_t v) {
    const int bits = v ? 64 - __clzll(v) : 1;
    return (uint32_t)((bits + 6) / 7);
}

__device__ __forceinline__ uint32_t run_digits(uint64_t v) {
    uint32_t d = 1;
    uint64_t p = 10;
    while (d < 20 && v >= p) {
        ++d;
        p *= 10;
    }
    return d;
}

__global__ void __launch_bounds__(kRunThreads) pb_run_encode_kernel(const PbRunChunk* __restrict__ chunks,
                                                                    int32_t* __restrict__ err) {
    __shared__ uint8_t image[kPbRunChunkElems * kRunMaxElemBytes];
    __shared__ uint32_t wave_tot[kRunThreads / 64];
    __shared__ uint32_t round_base;
    const PbRunChunk c = chunks[blockIdx.x];
    const int t = threadIdx.x, wave = t >> 6;
    const bool decimal = c.format == PB_RUN_DECIMAL;
    if (t == 0) round_base = 0;
    __syncthreads();
    const uint32_t count = c.count < kPbRunChunkElems ? c.count : kPbRunChunkElems;
    // every round's element is loaded before any is used: from pinned host
    // memory each load is a PCIe round trip, so the 8 go out together
    // instead of one per round behind the scan's barriers
    constexpr int kRounds = kPbRunChunkElems / kRunThreads;
    uint64_t raws[kRounds];
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const uint32_t i = (uint32_t)r * kRunThreads + t;
        raws[r] = i < count ? run_load(c.src, i, c.kind) : 0;
    }
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const uint32_t r0 = (uint32_t)r * kRunThreads;
        if (r0 >= count) break;
        const uint32_t i = r0 + t;
        uint32_t len = 0;
        uint64_t v = 0;
        bool neg = false;
        if (i < count) {
            if (!decimal) {
                v = run_value(raws[r], c.kind);
                len = run_varint_len(v);
            } else if (c.kind == PB_RUN_BOOL) {
                v = raws[r];
                len = v ? 4 : 5;
            } else {
                neg = run_negative(raws[r], c.kind, &v);
                len = run_digits(v) + (neg ? 1 : 0);
            }
            if (decimal && !(c.last && i + 1 == count)) len += 1;  // ','
        }
        // block exclusive scan of len in element order: the two halves of
        // wg::block_excl_scan with the tail written out. wg::scan_rank's
        // unrolled form costs this kernel 10 VGPRs (57 -> 67), a wave per SIMD
        const uint32_t incl = wg::scan_post(len, wave_tot);
        __syncthreads();
        uint32_t pos = round_base + incl - len;
        for (int w = 0; w < wave; ++w) pos += wave_tot[w];
        const uint32_t round_total = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
        if (i < count) {
            uint8_t* o = image + pos;
            if (!decimal) {
                for (uint32_t j = 0; j < len; ++j) {
                    o[j] = (uint8_t)((v & 0x7f) | (j + 1 < len ? 0x80 : 0));
                    v >>= 7;
                }
            } else if (c.kind == PB_RUN_BOOL) {
                const char* s = v ? "true" : "false";
                const uint32_t n = v ? 4 : 5;
                for (uint32_t j = 0; j < n; ++j) o[j] = (uint8_t)s[j];
                if (len > n) o[n] = ',';
            } else {
                const uint32_t nd = run_digits(v);
                uint32_t k = 0;
                if (neg) o[k++] = '-';
                for (uint32_t j = 0; j < nd; ++j) {
                    const uint64_t q = v / 10;
                    o[k + nd - 1 - j] = (uint8_t)('0' + (uint32_t)(v - q * 10));
                    v = q;
                }
                k += nd;
                if (len > k) o[k] = ',';
            }
        }
        __syncthreads();  // wave_tot is rewritten by the next round
        if (t == 0) round_base += round_total;
        __syncthreads();
    }
    const uint32_t total = round_base;
    if (total != c.bytes) {
        if (t == 0) err[blockIdx.x] = 1;
        return;
    }
    wg::copy_out_bytes<kRunThreads>(image, c.dst, total);
    if (t == 0) err[blockIdx.x] = 0;
}

// ------------------------------------------------------------ run decoder
// Packed fields of a decoded body (the reference's ParsePbFromIOBuf walks
// them element by element on the host, src/brpc/protocol.cpp).
// Both passes read the chunk (plus up to 16 bytes of the run before it)
// with 16-byte loads of the aligned span around it (the decode pass through
// wg::stage16): a wave's load moves 1 KiB instead of the 64 bytes of per-lane
// byte loads, which held the count pass to ~1 TB/s on HBM. Lane t then owns
// chunk bytes [16t, 16t + 16) of the staged copy.
constexpr int kHalo = 16;
// staged at raw + kPad: every lane's 32-byte window (16 bytes before its
// own 16) stays inside the array
constexpr int kPad = 16;
constexpr int kStage16 = (kPad + kHalo + kPbRunDecodeChunkBytes + 64) / 16;
static_assert((kHalo + kPbRunDecodeChunkBytes + 15 + 15) / 16 <= 2 * kRunThreads, "two rounds of loads stage a chunk");

// Bits 0..3 of each nibble k: byte k of w ends a varint (top bit clear).
__device__ __forceinline__ uint32_t ends_of(uint32_t w) {
    const uint32_t m = ~w & 0x80808080u;
    return ((m >> 7) & 1) | ((m >> 14) & 2) | ((m >> 21) & 4) | ((m >> 28) & 8);
}

__global__ void __launch_bounds__(kRunThreads) pb_run_count_kernel(const PbRunDecodeChunk* __restrict__ chunks,
                                                                   int nchunks, uint32_t* __restrict__ counts,
                                                                   uint32_t* __restrict__ prefix) {
    // one wave per chunk, straight from the loads (no LDS, no barriers):
    // varint ends are bytes with the top bit clear, counted 16 at a time
    // inside [0, len). Every lane issues its (up to 5) 16-byte loads before
    // using any, so a wave keeps a whole 4 KiB chunk in flight; one load per
    // lane and a block-wide reduction per chunk held this pass to ~1 TB/s
    constexpr int kUnits = (kPbRunDecodeChunkBytes + 16 + 63 * 16) / (64 * 16);  // 16 B units per lane
    const int lane = threadIdx.x & 63;
    const int nwaves = (int)gridDim.x * (kRunThreads / 64);
    for (int ci = (int)blockIdx.x * (kRunThreads / 64) + (int)(threadIdx.x >> 6); ci < nchunks; ci += nwaves) {
        const PbRunDecodeChunk c = chunks[ci];
        const uint32_t len = c.len < kPbRunDecodeChunkBytes ? c.len : kPbRunDecodeChunkBytes;
        const uint8_t* p = c.run + c.offset;
        const int a = (int)((uintptr_t)p & 15);
        const u32x4* src = reinterpret_cast<const u32x4*>(p - a);
        const uint32_t n16 = ((uint32_t)a + len + 15) >> 4;
        u32x4 v[kUnits];
#pragma unroll
        for (int k = 0; k < kUnits; ++k) {
            const uint32_t i = (uint32_t)lane + 64u * k;
            if (i < n16) v[k] = src[i];
        }
        uint32_t n = 0;
#pragma unroll
        for (int k = 0; k < kUnits; ++k) {
            const uint32_t i = (uint32_t)lane + 64u * k;
            if (i < n16) {
                const uint32_t bits =
                    ends_of(v[k].x) | (ends_of(v[k].y) << 4) | (ends_of(v[k].z) << 8) | (ends_of(v[k].w) << 12);
                const int lo = max(a - (int)(i * 16), 0), hi = min(a + (int)len - (int)(i * 16), 16);
                if (hi > lo) n += __popc(bits & (((1u << hi) - 1) & ~((1u << lo) - 1)));
            }
        }
        n = wg::wave_sum(n);
        if (lane == 0) {
            counts[ci] = n;  // the host's copy (pinned)
            prefix[ci] = n;  // scanned in HBM by pb_run_prefix_kernel
        }
    }
}

// One workgroup turns the per-chunk counts into their exclusive prefix sum
// over the whole table (mod 2^32), so every chunk of every run finds its
// first element index as prefix[chunk] - prefix[run's first chunk] with two
// loads: summing the earlier chunks' counts in each workgroup instead grows
// with the square of a run's length (16 K chunks for a 64 MiB run).
constexpr int kPrefixThreads = 1024, kPrefixPer = 4;
__global__ void __launch_bounds__(kPrefixThreads) pb_run_prefix_kernel(uint32_t* __restrict__ prefix, int n) {
    __shared__ uint32_t wave_tot[kPrefixThreads / 64];
    const int t = threadIdx.x;
    uint32_t carry = 0;
    for (int base = 0; base < n; base += kPrefixThreads * kPrefixPer) {
        const int i0 = base + t * kPrefixPer;
        uint32_t v[kPrefixPer], mine = 0;
#pragma unroll
        for (int j = 0; j < kPrefixPer; ++j) {
            v[j] = i0 + j < n ? prefix[i0 + j] : 0;
            mine += v[j];
        }
        uint32_t tile;
        uint32_t run = carry + wg::block_excl_scan<kPrefixThreads>(mine, wave_tot, &tile);
#pragma unroll
        for (int j = 0; j < kPrefixPer; ++j) {
            if (i0 + j < n) prefix[i0 + j] = run;
            run += v[j];
        }
        carry += tile;
        __syncthreads();  // wave_tot is rewritten by the next tile
    }
}

__device__ __forceinline__ void store_elem(uint8_t* o, uint32_t kind, uint64_t raw) {
    switch (kind) {
    case PB_RUN_INT32:
    case PB_RUN_UINT32: *reinterpret_cast<uint32_t*>(o) = (uint32_t)raw; break;
    case PB_RUN_SINT32: {
        const uint32_t u = (uint32_t)raw;
        *reinterpret_cast<int32_t*>(o) = (int32_t)(u >> 1) ^ -(int32_t)(u & 1);
        break;
    }
    case PB_RUN_SINT64: *reinterpret_cast<int64_t*>(o) = (int64_t)(raw >> 1) ^ -(int64_t)(raw & 1); break;
    case PB_RUN_BOOL: *o = raw ? 1 : 0; break;
    default: *reinterpret_cast<uint64_t*>(o) = raw; break;
    }
}

__global__ void __launch_bounds__(kRunThreads) pb_run_decode_kernel(const PbRunDecodeChunk* __restrict__ chunks,
                                                                    int nchunks,
                                                                    const uint32_t* __restrict__ prefix,
                                                                    int32_t* __restrict__ err) {
    __shared__ u32x4 raw[kStage16];
    __shared__ __attribute__((aligned(16))) uint8_t image[kPbRunDecodeChunkBytes * 8 + 16];
    __shared__ uint32_t wave_tot[kRunThreads / 64];
    __shared__ int bad;
    const int t = threadIdx.x;
    PbRunDecodeChunk c = chunks[blockIdx.x];
    // grid-stride over the chunks; the next descriptor (pinned host memory)
    // is fetched while this chunk decodes
    for (int ci = blockIdx.x; ci < nchunks; ci += gridDim.x) {
        PbRunDecodeChunk next = c;
        if (ci + (int)gridDim.x < nchunks) next = chunks[ci + gridDim.x];
        const uint32_t len = c.len < kPbRunDecodeChunkBytes ? c.len : kPbRunDecodeChunkBytes;
        const uint32_t halo = c.offset < (uint32_t)kHalo ? c.offset : (uint32_t)kHalo;
        if (t == 0) bad = 0;
        // chunk byte x (x in [-halo, len)) is at LDS byte x + o
        const uint32_t o = kPad + wg::stage16<kRunThreads, 2>(c.run + c.offset - halo, halo + len, raw + kPad / 16) + halo;
        // first element index: the earlier chunks of the run
        const uint32_t base = prefix[ci] - prefix[c.first];
        const uint32_t eb = c.kind == PB_RUN_BOOL ? 1 : (c.kind <= PB_RUN_SINT32 ? 4 : 8);
        uint8_t* dst = static_cast<uint8_t*>(c.dst) + (size_t)base * eb;
        // the image sits at dst's alignment so copy-out is 16-byte both sides;
        // element stores stay naturally aligned only when dst is
        const uint32_t sh0 = (uint32_t)((uintptr_t)dst & 15);
        const uint32_t sh = sh0 % eb == 0 ? sh0 : 0;
        __syncthreads();  // the staging is complete
        // lane t decodes the varints ending in chunk bytes [j0, j0 + 16), from a
        // register window of bytes [j0 - 16, j0 + 16): 9 aligned LDS words
        // funnel-shifted into 8, then fixed-position bit work only (no
        // byte-serial LDS walks)
        const uint32_t j0 = (uint32_t)t * 16;
        const uint32_t wb = o + j0 - 16;  // >= 0: o >= kPad
        const uint32_t* words = reinterpret_cast<const uint32_t*>(raw) + (wb >> 2);
        const uint32_t fs = (wb & 3) * 8;
        uint32_t W[8];
        {
            uint32_t w9[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) w9[k] = words[k];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                W[k] = fs ? wg::funnel(w9[k], w9[k + 1], fs) : w9[k];
            }
        }
        uint32_t cont = 0;  // bit i: window byte i carries a continuation bit
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t m = W[k] & 0x80808080u;
            cont |= (((m >> 7) & 1) | ((m >> 14) & 2) | ((m >> 21) & 4) | ((m >> 28) & 8)) << (4 * k);
        }
        // bytes before the run's staged part end the lookback (the first lane of
        // a run's first chunk)
        const int first_valid = 16 - (int)j0 - (int)halo;  // window index of chunk byte -halo
        if (first_valid > 0) cont &= ~((1u << first_valid) - 1);
        const int mine_n = (int)len - (int)j0;
        const uint32_t own = mine_n >= 16 ? 0xFFFFu : (mine_n <= 0 ? 0u : ((1u << mine_n) - 1));
        const uint32_t term = (~cont >> 16) & own;
        const uint32_t mine = __popc(term);
        uint32_t total;
        uint32_t rank = wg::block_excl_scan<kRunThreads>(mine, wave_tot, &total);
#define WBYTE(i) ((W[(i) >> 2] >> (8 * ((i) & 3))) & 0xFFu)
#pragma unroll
        for (int p = 16; p < 32; ++p) {
            if (!((term >> (p - 16)) & 1)) continue;
            const uint32_t below = ~cont & ((1u << p) - 1);
            const int n = p - (below ? 31 - __clz(below) : -1);  // varint bytes
            if (n > 10 || (n == 10 && WBYTE(p) > 1)) bad = 1;
            uint64_t v = 0;
#pragma unroll
            for (int k = 0; k < 10; ++k) {
                if (k < n) v = (v << 7) | (WBYTE(p - k) & 0x7F);
            }
            store_elem(image + sh + (size_t)rank * eb, c.kind, v);
            ++rank;
        }
#undef WBYTE
        __syncthreads();
        if (bad) {
            if (t == 0) err[ci] = 1;
        } else {
            const uint32_t nbytes = total * eb;
            if (sh == sh0) {
                wg::copy_out_phased<kRunThreads>(image, sh, dst, nbytes);
            } else {
                wg::copy_out_bytes<kRunThreads>(image, dst, nbytes);
            }
            if (t == 0) err[ci] = 0;
        }
        __syncthreads();  // raw, image, wave_tot and bad are reused
        c = next;
    }
}

// --------------------------------------------------------- message builder
// Arrays in HBM -> serialized messages in HBM (kernels.h: size, prefix,
// layout, place). The host knows no value, so nothing here takes a size from
// it: the size pass measures every chunk, the prefix kernel above turns the
// sizes into offsets within each field, and the layout pass adds the headers.
constexpr int kMsgImage16 = (kPbRunChunkElems * 10 + 16 + 15) / 16;  // a numeric chunk at any 16-byte phase
static_assert(kMsgImage16 * 16 >= (int)kPbMsgBytesChunk + 32, "a bytes chunk is staged in the same image");

__device__ __forceinline__ uint32_t msg_chunk_count(const PbMsgChunk& c) {
    const uint32_t most = c.kind == PB_MSG_BYTES ? kPbMsgBytesChunk : kPbRunChunkElems;
    return c.count < most ? c.count : most;
}

// A lane's share of the encoded size of a numeric chunk whose source is
// 16-byte aligned, read as 16-byte units (2 or 4 elements each; unit u goes
// to lane u % 64). The last unit may reach past the chunk's last element:
// inside its aligned 16 bytes, so inside its page.
template <int kElemBytes>
__device__ __forceinline__ uint32_t msg_size_units(const void* src_, uint32_t count, uint32_t kind, int lane) {
    constexpr int kIn = 16 / kElemBytes;
    constexpr int kUnits = kPbRunChunkElems / kIn / 64;
    const u32x4* src = static_cast<const u32x4*>(src_);
    const uint32_t nunits = (count + kIn - 1) / kIn;
    u32x4 v[kUnits];
#pragma unroll
    for (int k = 0; k < kUnits; ++k) {
        const uint32_t u = (uint32_t)lane + 64u * k;
        if (u < nunits) v[k] = src[u];
    }
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < kUnits; ++k) {
        const uint32_t u = (uint32_t)lane + 64u * k;
        if (u >= nunits) continue;
        const uint32_t w[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
        for (int j = 0; j < kIn; ++j) {
            if (u * kIn + j >= count) continue;
            uint64_t raw;  // as run_load makes it
            if (kElemBytes == 8) {
                raw = ((uint64_t)w[2 * j + 1] << 32) | w[2 * j];
            } else {
                raw = kind == PB_RUN_UINT32 ? (uint64_t)w[j] : (uint64_t)(int64_t)(int32_t)w[j];
            }
            n += run_varint_len(run_value(raw, kind));
        }
    }
    return n;
}

__global__ void __launch_bounds__(kRunThreads) pb_msg_size_kernel(const PbMsgChunk* __restrict__ chunks, int nchunks,
                                                                  uint32_t* __restrict__ sizes) {
    // one wave per chunk, no LDS, no barriers. A lane's share of the chunk
    // is all loaded before any of it is used, so a wave keeps its whole chunk
    // (16 KiB of 64-bit elements) in flight: the pass only reads, it is bound
    // by HBM. 16-byte loads when the source allows them, else one element each
    constexpr int kPer = kPbRunChunkElems / 64;
    const int lane = threadIdx.x & 63;
    const int nwaves = (int)gridDim.x * (kRunThreads / 64);
    if (blockIdx.x == 0 && threadIdx.x == 0) sizes[nchunks] = 0;  // becomes the total under the scan
    for (int ci = (int)blockIdx.x * (kRunThreads / 64) + (int)(threadIdx.x >> 6); ci < nchunks; ci += nwaves) {
        const PbMsgChunk c = chunks[ci];
        const uint32_t count = msg_chunk_count(c);
        uint32_t n = count;  // bools and raw bytes: one byte each
        if (c.kind < PB_RUN_BOOL) {
            if (((uintptr_t)c.src & 15) == 0) {
                n = c.kind <= PB_RUN_SINT32 ? msg_size_units<4>(c.src, count, c.kind, lane)
                                            : msg_size_units<8>(c.src, count, c.kind, lane);
            } else {
                uint64_t raws[kPer];
#pragma unroll
                for (int k = 0; k < kPer; ++k) {
                    const uint32_t i = (uint32_t)lane + 64u * k;
                    raws[k] = i < count ? run_load(c.src, i, c.kind) : 0;
                }
                n = 0;
#pragma unroll
                for (int k = 0; k < kPer; ++k) {
                    const uint32_t i = (uint32_t)lane + 64u * k;
                    if (i < count) n += run_varint_len(run_value(raws[k], c.kind));
                }
            }
            n = wg::wave_sum(n);
        }
        if (lane == 0) sizes[ci] = n;
    }
}

__device__ __forceinline__ uint32_t put_varint(uint8_t* o, uint64_t v) {
    uint32_t n = 0;
    while (v >= 0x80) {
        o[n++] = (uint8_t)(v | 0x80);
        v >>= 7;
    }
    o[n++] = (uint8_t)v;
    return n;
}

// Payload and header length of field f (payloads stay below 2^32: the host
// refuses a field whose worst case does not).
__device__ __forceinline__ void msg_field_lens(const PbMsgField& f, const uint32_t* prefix, uint32_t* plen,
                                               uint32_t* hlen) {
    *plen = prefix[f.first_chunk + f.nchunks] - prefix[f.first_chunk];
    *hlen = f.headerless ? 0 : run_varint_len(f.tag) + run_varint_len(*plen);
}

// One wave per message: field k's header starts where fields 0..k-1 end.
// The length is summed first, so a message that does not fit gets no byte.
__global__ void __launch_bounds__(64) pb_msg_layout_kernel(const PbMsgJob* __restrict__ msgs,
                                                           const PbMsgField* __restrict__ fields,
                                                           const uint32_t* __restrict__ prefix,
                                                           uint64_t* __restrict__ base, PbMsgResult* __restrict__ res,
                                                           PbMsgFieldResult* __restrict__ fres) {
    const PbMsgJob m = msgs[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    uint64_t total = 0;
    for (uint32_t f0 = 0; f0 < m.nfields; f0 += 64) {
        uint64_t mine = 0;
        if (f0 + lane < m.nfields) {
            uint32_t plen, hlen;
            msg_field_lens(fields[m.first_field + f0 + lane], prefix, &plen, &hlen);
            mine = (uint64_t)plen + hlen;
        }
        total += wg::wave_sum(mine);
    }
    const bool fits = total <= m.cap;
    uint64_t carry = 0;
    for (uint32_t f0 = 0; f0 < m.nfields; f0 += 64) {
        const bool live = f0 + lane < m.nfields;
        const uint32_t gf = m.first_field + f0 + lane;
        PbMsgField f;
        uint32_t plen = 0, hlen = 0;
        if (live) {
            f = fields[gf];
            msg_field_lens(f, prefix, &plen, &hlen);
        }
        const uint64_t mine = (uint64_t)plen + hlen;
        const uint64_t incl = wg::wave_incl_scan(mine);
        const uint64_t off = carry + incl - mine;
        if (live) {
            if (fits) {
                uint8_t* o = m.dst + off;
                if (!f.headerless) {
                    o += put_varint(o, f.tag);
                    put_varint(o, plen);
                }
                base[gf] = (uint64_t)(uintptr_t)(m.dst + off + hlen);
                fres[gf] = PbMsgFieldResult{off + hlen, plen};
            } else {
                base[gf] = 0;  // the place pass skips the field's chunks
                fres[gf] = PbMsgFieldResult{0, 0};
            }
        }
        carry += __shfl(incl, 63, 64);
    }
    if (lane == 0) res[blockIdx.x] = PbMsgResult{total, fits ? 0 : 3, 0};
}

// One workgroup per chunk. A numeric chunk is encoded like
// pb_run_encode_kernel's varint path, into an LDS image that sits at the
// destination's 16-byte phase, so it leaves through wg::copy_out_phased. What
// the chunk encodes to is compared with what the size pass measured: the two
// differ only when the source changed in between, and then nothing is written
// (the offsets of every later chunk were derived from the measured size).
__global__ void __launch_bounds__(kRunThreads) pb_msg_place_kernel(const PbMsgChunk* __restrict__ chunks,
                                                                   const PbMsgField* __restrict__ fields,
                                                                   const uint32_t* __restrict__ prefix,
                                                                   const uint64_t* __restrict__ base,
                                                                   PbMsgResult* __restrict__ res) {
    __shared__ u32x4 image16[kMsgImage16];
    __shared__ uint32_t wave_tot[kPbRunChunkElems / kRunThreads][kRunThreads / 64];
    uint8_t* image = reinterpret_cast<uint8_t*>(image16);
    const uint32_t ci = blockIdx.x;
    const PbMsgChunk c = chunks[ci];
    const uint64_t b = base[c.field];
    if (!b) return;  // the message did not fit (the whole workgroup leaves)
    const uint32_t want = prefix[ci + 1] - prefix[ci];
    uint8_t* dst = reinterpret_cast<uint8_t*>((uintptr_t)(b + (uint32_t)(prefix[ci] - prefix[c.first])));
    const int t = threadIdx.x;
    const uint32_t count = msg_chunk_count(c);
    if (c.kind == PB_MSG_BYTES) {  // a straight copy through LDS
        constexpr int kUnits = (kPbMsgBytesChunk / 16 + 2 + kRunThreads - 1) / kRunThreads;
        const uint32_t a = wg::stage16<kRunThreads, kUnits>(static_cast<const uint8_t*>(c.src), count, image16);
        __syncthreads();
        if (((uintptr_t)dst & 15) == a) {
            wg::copy_out_phased<kRunThreads>(image, a, dst, count);
        } else {
            wg::copy_out_bytes<kRunThreads>(image + a, dst, count);
        }
        return;
    }
    const uint32_t sh = (uint32_t)((uintptr_t)dst & 15);
    constexpr int kRounds = kPbRunChunkElems / kRunThreads;
    uint64_t raws[kRounds];
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const uint32_t i = (uint32_t)r * kRunThreads + t;
        raws[r] = i < count ? run_load(c.src, i, c.kind) : 0;
    }
    // lane t of round r takes element 256r + t. Every round's lengths are
    // scanned inside the waves first, so the whole chunk needs two barriers
    // (the wave totals of all rounds, then the image), not three per round
    uint32_t lens[kRounds], incls[kRounds];
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const uint32_t i = (uint32_t)r * kRunThreads + t;
        raws[r] = run_value(raws[r], c.kind);
        lens[r] = i < count ? run_varint_len(raws[r]) : 0;
        incls[r] = wg::scan_post(lens[r], wave_tot[r]);
    }
    __syncthreads();
    uint32_t total = 0;
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const uint32_t before = total;  // the rounds in front of this one
        const uint32_t pos = before + wg::scan_rank<kRunThreads>(incls[r], lens[r], wave_tot[r], &total);
        uint8_t* o = image + sh + pos;
        uint64_t v = raws[r];
        for (uint32_t j = 0; j < lens[r]; ++j) {
            o[j] = (uint8_t)((v & 0x7f) | (j + 1 < lens[r] ? 0x80 : 0));
            v >>= 7;
        }
    }
    __syncthreads();
    if (total != want) {
        if (t == 0) res[fields[c.field].msg].err = 4;
        return;
    }
    wg::copy_out_phased<kRunThreads>(image, sh, dst, total);
}

// ---------------------------------------------------------- record builder
// Several columns -> the occurrences of one repeated sub-message with several
// fields (kernels.h: init, size, prefix, measure, prefix, heads, place; the
// wire rules are base/pb_records.h). One flat array + row ends -> one
// repeated field is the job of one column. No lane walks a row: a column's
// payload in a row is the difference of two byte prefixes, each a group
// prefix plus at most 63 element sizes. First the parts that see one column,
// a PbRowsJob, alone: the size pass and the body of the place pass.
constexpr int kRowsRounds = kPbRowsChunkElems / kRunThreads;
constexpr uint32_t kRowsFewRows = 16;  // a chunk meeting at most this many rows leaves segment by segment
constexpr uint32_t kNoRow = 0xFFFFFFFFu;

__global__ void __launch_bounds__(kRunThreads) pb_rows_size_kernel(const PbRowsJob* __restrict__ jobs, int njobs,
                                                                   uint32_t* __restrict__ groups) {
    const PbRowsJob job = jobs[wg::job_of<&PbRowsJob::first_chunk>(jobs, njobs, blockIdx.x)];
    if (!pb_rows::IsVarintKind(job.kind)) return;
    const uint32_t cs = (blockIdx.x - job.first_chunk) * kPbRowsChunkElems;
    const uint32_t n = job.count - cs < kPbRowsChunkElems ? job.count - cs : kPbRowsChunkElems;
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    // a wave's 64 elements of a round are one group; all loads go out first
    uint64_t v[kRowsRounds];
#pragma unroll
    for (int r = 0; r < kRowsRounds; ++r) {
        const uint32_t i = (uint32_t)r * kRunThreads + t;
        v[r] = i < n ? pb_rows::WireValue(job.src, (uint64_t)cs + i, job.kind) : 0;
    }
#pragma unroll
    for (int r = 0; r < kRowsRounds; ++r) {
        const uint32_t i = (uint32_t)r * kRunThreads + t;
        const uint32_t len = wg::wave_sum(i < n ? run_varint_len(v[r]) : 0u);
        const uint32_t g0 = (uint32_t)r * kRunThreads + wave * 64;  // the group's first element in the chunk
        if (lane == 0 && g0 < n) groups[job.first_group + (cs + g0) / kPbRowsGroupElems] = len;
    }
}

// Encoded bytes of elements [0, e) of the job, e <= count.
__device__ __forceinline__ uint32_t rows_bytes_before(const PbRowsJob& job, const uint32_t* groups, uint32_t e) {
    if (!pb_rows::IsVarintKind(job.kind)) return e * pb_rows::SourceBytes(job.kind);
    uint32_t b = groups[job.first_group + e / kPbRowsGroupElems] - groups[job.first_group];
    for (uint32_t i = e & ~(kPbRowsGroupElems - 1); i < e; ++i) {
        b += run_varint_len(pb_rows::WireValue(job.src, i, job.kind));
    }
    return b;
}

// Entry r of a table of row ends. A scalar column comes without one (kIota):
// element r is row r.
template <bool kIota>
__device__ __forceinline__ uint32_t rows_end_at(const uint32_t* ends, uint64_t r) {
    if (kIota && !ends) return (uint32_t)r + 1;
    return ends[r];
}

// The place pass of one chunk of one column of a record job whose rows were measured and whose message of `total` bytes fits: delta[r]
// is the distance from "bytes before element e" to "offset of element e in
// dst" for row r. *err = 4 below: a source (or row_ends) changed under the
// builder's hands, seen as a size that no longer matches or a store that
// would leave the message.
template <bool kIota>
__device__ __forceinline__ void rows_place_chunk(const PbRowsJob& job, uint32_t chunk, uint32_t total,
                                                 const uint32_t* __restrict__ groups,
                                                 const uint32_t* __restrict__ delta, int32_t* err) {
    __shared__ u32x4 image16[kMsgImage16];
    // few rows: the position of every element in the image (and the total);
    // many rows: the row of every element, relative to the chunk's first
    __shared__ uint32_t aux[kPbRowsChunkElems + 1];
    __shared__ uint32_t wave_tot[kRowsRounds][kRunThreads / 64];
    __shared__ uint32_t wave_max[kRunThreads / 64];
    uint8_t* image = reinterpret_cast<uint8_t*>(image16);
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t cs = chunk * kPbRowsChunkElems;
    const uint32_t n = job.count - cs < kPbRowsChunkElems ? job.count - cs : kPbRowsChunkElems;
    const uint32_t ce = cs + n;
    const uint32_t* ends = job.row_ends;
    // the rows that hold the chunk's first and last element
    uint32_t lo = 0, hi = job.rows - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (rows_end_at<kIota>(ends, mid) > cs) {
            hi = mid;
        } else {
            lo = mid + 1;
        }
    }
    const uint32_t r_lo = lo;
    hi = job.rows - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (rows_end_at<kIota>(ends, mid) >= ce) {
            hi = mid;
        } else {
            lo = mid + 1;
        }
    }
    const uint32_t r_hi = lo;

    const bool varints = pb_rows::IsVarintKind(job.kind);
    const uint32_t w = pb_rows::SourceBytes(job.kind);
    uint64_t vals[kRowsRounds];
#pragma unroll
    for (int r = 0; r < kRowsRounds; ++r) {
        const uint32_t i = (uint32_t)r * kRunThreads + t;
        vals[r] = i < n ? pb_rows::WireValue(job.src, (uint64_t)cs + i, job.kind) : 0;
    }
    // every element's size and its position among the chunk's bytes
    uint32_t lens[kRowsRounds], poss[kRowsRounds];
    uint32_t before_cs, want, bytes = 0;
    if (varints) {
        const uint32_t g0 = groups[job.first_group];
        before_cs = groups[job.first_group + cs / kPbRowsGroupElems] - g0;
        const uint32_t gend = ce == job.count ? job.count / kPbRowsGroupElems + 1 : ce / kPbRowsGroupElems;
        want = groups[job.first_group + gend] - g0 - before_cs;
#pragma unroll
        for (int r = 0; r < kRowsRounds; ++r) {
            const uint32_t i = (uint32_t)r * kRunThreads + t;
            lens[r] = i < n ? run_varint_len(vals[r]) : 0;
            poss[r] = wg::scan_post(lens[r], wave_tot[r]);  // the wave's inclusive scan until the barrier
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kRowsRounds; ++r) {
            const uint32_t before = bytes;  // the rounds in front of this one
            poss[r] = before + wg::scan_rank<kRunThreads>(poss[r], lens[r], wave_tot[r], &bytes);
        }
    } else {
        before_cs = cs * w;
        want = bytes = n * w;
#pragma unroll
        for (int r = 0; r < kRowsRounds; ++r) {
            const uint32_t i = (uint32_t)r * kRunThreads + t;
            lens[r] = i < n ? w : 0;
            poss[r] = i * w;
        }
    }
    if (bytes != want) {
        if (t == 0) *err = 4;
        return;
    }

    if (r_hi - r_lo < kRowsFewRows) {
        // the image sits at the 16-byte phase of the chunk's first byte in dst
        // (the first row's segment always leaves aligned, a chunk inside one
        // row entirely)
        uint32_t sh = (uint32_t)((uintptr_t)(job.dst + (uint32_t)(delta[r_lo] + before_cs)) & 15);
        if (sh % w) sh = 0;
#pragma unroll
        for (int r = 0; r < kRowsRounds; ++r) {
            const uint32_t i = (uint32_t)r * kRunThreads + t;
            if (i >= n) continue;
            uint8_t* o = image + sh + poss[r];
            if (varints) {
                uint64_t v = vals[r];
                for (uint32_t k = 0; k < lens[r]; ++k) {
                    o[k] = (uint8_t)((v & 0x7f) | (k + 1 < lens[r] ? 0x80 : 0));
                    v >>= 7;
                }
                aux[i] = poss[r];
            } else if (w == 1) {
                *o = (uint8_t)vals[r];
            } else if (w == 4) {
                *reinterpret_cast<uint32_t*>(o) = (uint32_t)vals[r];
            } else {
                *reinterpret_cast<uint64_t*>(o) = vals[r];
            }
        }
        if (t == 0 && varints) aux[n] = bytes;
        __syncthreads();
        for (uint32_t row = r_lo; row <= r_hi; ++row) {
            uint32_t s = row ? rows_end_at<kIota>(ends, row - 1) : 0, e = rows_end_at<kIota>(ends, row);
            s = s > cs ? s : cs;
            e = e < ce ? e : ce;
            if (e <= s) continue;
            const uint32_t a = varints ? aux[s - cs] : (s - cs) * w;
            const uint32_t b = varints ? aux[e - cs] : (e - cs) * w;
            const uint32_t off = delta[row] + before_cs + a;
            if (b < a || (uint64_t)off + (b - a) > total) {
                if (t == 0) *err = 4;
                continue;
            }
            uint8_t* d = job.dst + off;
            if (((uint32_t)(uintptr_t)d & 15) == ((sh + a) & 15)) {
                wg::copy_out_phased<kRunThreads>(image, sh + a, d, b - a);
            } else {
                wg::copy_out_bytes<kRunThreads>(image + sh + a, d, b - a);
            }
        }
        return;
    }

    // many rows: every nonempty row that starts in the chunk (the first may
    // start before it) marks its first element; a max-scan spreads the marks
    for (uint32_t i = t; i < n; i += kRunThreads) aux[i] = 0;
    __syncthreads();
    for (uint64_t row = (uint64_t)r_lo + t; row <= r_hi; row += kRunThreads) {
        const uint32_t s = row ? rows_end_at<kIota>(ends, row - 1) : 0, e = rows_end_at<kIota>(ends, row);
        if (e <= s) continue;
        const uint32_t i = s > cs ? s - cs : 0;
        if (i < n) aux[i] = (uint32_t)(row - r_lo) + 1;
    }
    __syncthreads();
    {
        constexpr uint32_t kPer = kPbRowsChunkElems / kRunThreads;  // consecutive elements per thread
        uint32_t m[kPer], run = 0;
#pragma unroll
        for (uint32_t k = 0; k < kPer; ++k) {
            const uint32_t i = t * kPer + k;
            const uint32_t x = i < n ? aux[i] : 0;
            run = run > x ? run : x;
            m[k] = run;
        }
        const uint32_t incl = wg::wave_incl_scan(run, [](uint32_t a, uint32_t b) { return a > b ? a : b; });
        if (lane == 63) wave_max[wave] = incl;
        uint32_t carry = wg::wave_prev(incl);
        if (lane == 0) carry = 0;
        __syncthreads();
        for (uint32_t k = 0; k < wave; ++k) carry = carry > wave_max[k] ? carry : wave_max[k];
#pragma unroll
        for (uint32_t k = 0; k < kPer; ++k) {
            const uint32_t i = t * kPer + k;
            if (i < n) aux[i] = m[k] > carry ? m[k] : carry;
        }
    }
    __syncthreads();
    bool changed = false;
#pragma unroll
    for (int r = 0; r < kRowsRounds; ++r) {
        const uint32_t i = (uint32_t)r * kRunThreads + t;
        if (i >= n) continue;
        const uint32_t mark = aux[i];
        if (mark == 0 || mark - 1 > r_hi - r_lo) {
            changed = true;
            continue;
        }
        const uint32_t off = delta[r_lo + (mark - 1)] + before_cs + poss[r];
        if ((uint64_t)off + lens[r] > total) {
            changed = true;
            continue;
        }
        uint8_t* o = job.dst + off;
        uint64_t v = vals[r];
        if (varints) {
            for (uint32_t k = 0; k < lens[r]; ++k) {
                o[k] = (uint8_t)((v & 0x7f) | (k + 1 < lens[r] ? 0x80 : 0));
                v >>= 7;
            }
        } else {
            for (uint32_t k = 0; k < w; ++k) {
                o[k] = (uint8_t)v;
                v >>= 8;
            }
        }
    }
    if (changed) *err = 4;
}

// The passes that see a record job: a row's size sums over its columns, and
// each column has its own delta.
constexpr uint64_t kNoRecord = ~0ull;  // the offender key: row << 4 | column

__global__ void __launch_bounds__(64) pb_records_init_kernel(const PbRecordsJob* __restrict__ jobs, int njobs,
                                                             const PbRowsJob* __restrict__ cols, int ncols,
                                                             PbRecordsJob* __restrict__ jobs_dev,
                                                             PbRowsJob* __restrict__ cols_dev,
                                                             uint32_t* __restrict__ groups,
                                                             unsigned long long* __restrict__ bad) {
    const int i = (int)(blockIdx.x * 64 + threadIdx.x);
    if (i < njobs) {
        jobs_dev[i] = jobs[i];
        bad[i] = kNoRecord;
    }
    if (i >= ncols) return;
    const PbRowsJob col = cols[i];
    cols_dev[i] = col;
    if (pb_rows::IsVarintKind(col.kind)) {
        // the group behind the last element (written again by the size pass
        // when it holds elements) and the one whose prefix is the total
        const uint32_t g = col.first_group + col.count / kPbRowsGroupElems;
        groups[g] = 0;
        groups[g + 1] = 0;
    }
}

__global__ void __launch_bounds__(kPbRowsBlockRows) pb_records_measure_kernel(
    const PbRecordsJob* __restrict__ jobs, int njobs, const PbRowsJob* __restrict__ cols,
    const uint32_t* __restrict__ groups, uint32_t* __restrict__ row_size, uint32_t* __restrict__ col_pay,
    uint32_t* __restrict__ col_delta, uint32_t* __restrict__ block_off, unsigned long long* __restrict__ bad) {
    __shared__ uint32_t wave_tot[kPbRowsBlockRows / 64];
    const int j = wg::job_of<&PbRecordsJob::first_rblock>(jobs, njobs, blockIdx.x);
    const PbRecordsJob job = jobs[j];
    const uint32_t block = blockIdx.x - job.first_rblock;
    const uint64_t r64 = (uint64_t)block * kPbRowsBlockRows + threadIdx.x;
    const uint32_t r = (uint32_t)r64;
    uint32_t size = 0;
    if (r64 < job.rows) {
        uint32_t fields = 0;
        for (uint32_t c = 0; c < job.ncols; ++c) {
            const PbRowsJob col = cols[job.first_col + c];
            const bool scalar = col.row_ends == nullptr;
            uint32_t s = r, e = r + 1;  // a scalar column: host-checked count == rows
            if (!scalar) {
                s = r ? col.row_ends[r - 1] : 0;
                e = col.row_ends[r];
                if (e < s || (r + 1 == job.rows && e != col.count)) atomicMin(&bad[j], ((unsigned long long)r << 4) | c);
                // a malformed table gets nothing written; until then it must
                // not make a lane read past the source
                s = s < col.count ? s : col.count;
                e = e < col.count ? e : col.count;
                e = e < s ? s : e;
            }
            const uint32_t before = rows_bytes_before(col, groups, s);
            const uint32_t p = rows_bytes_before(col, groups, e) - before;
            const uint32_t at = col.first_row + r;
            col_pay[at] = p;
            col_delta[at] = before;
            fields += p + pb_records::FieldHeaderBytes(col.inner, col.kind, scalar, p);
        }
        size = fields + pb_records::RowHeaderBytes(job.number, fields);
        row_size[job.first_row + r] = size;
    }
    uint32_t sum;
    wg::block_excl_scan<(int)kPbRowsBlockRows>(size, wave_tot, &sum);
    if (threadIdx.x == 0) {
        // the job's blocks, then one entry that becomes its total under the scan
        const uint32_t at = blockIdx.x + (uint32_t)j;
        block_off[at] = sum;
        if ((uint64_t)(block + 1) * kPbRowsBlockRows >= job.rows) block_off[at + 1] = 0;
    }
}

// The job's serialized size, from the scanned block sums.
__device__ __forceinline__ uint32_t records_job_total(const PbRecordsJob& job, int j, const uint32_t* block_off) {
    const uint32_t first = job.first_rblock + (uint32_t)j;
    const uint32_t nblocks = (uint32_t)(((uint64_t)job.rows + kPbRowsBlockRows - 1) / kPbRowsBlockRows);
    return block_off[first + nblocks] - block_off[first];
}

__global__ void __launch_bounds__(kPbRowsBlockRows) pb_records_heads_kernel(
    const PbRecordsJob* __restrict__ jobs, int njobs, const PbRowsJob* __restrict__ cols,
    const uint32_t* __restrict__ row_size, const uint32_t* __restrict__ col_pay, uint32_t* __restrict__ col_delta,
    const uint32_t* __restrict__ block_off, const unsigned long long* __restrict__ bad,
    PbRecordsResult* __restrict__ res) {
    __shared__ uint32_t wave_tot[kPbRowsBlockRows / 64];
    const int j = wg::job_of<&PbRecordsJob::first_rblock>(jobs, njobs, blockIdx.x);
    const PbRecordsJob job = jobs[j];
    const uint64_t r64 = (uint64_t)(blockIdx.x - job.first_rblock) * kPbRowsBlockRows + threadIdx.x;
    const bool live = r64 < job.rows;
    const uint32_t r = (uint32_t)r64;
    const unsigned long long key = bad[j];
    const uint32_t total = records_job_total(job, j, block_off);
    const bool ok = key == kNoRecord && total <= job.cap;
    if (r64 == 0) {
        res[j] = PbRecordsResult{total, key != kNoRecord ? (uint32_t)(key >> 4) : kNoRow,
                                 key != kNoRecord ? (uint32_t)(key & 15) : kNoRow,
                                 key != kNoRecord ? 1 : (total > job.cap ? 3 : 0)};
    }
    if (!ok) return;  // the whole workgroup
    // the row's offset: the blocks before this one, then the rows before it here
    uint32_t block_size;
    uint32_t off = wg::block_excl_scan<(int)kPbRowsBlockRows>(live ? row_size[job.first_row + r] : 0u, wave_tot,
                                                               &block_size);
    if (!live) return;
    off += block_off[blockIdx.x + (uint32_t)j] - block_off[job.first_rblock + (uint32_t)j];
    // a field's header follows from its payload size alone (an omitted packed
    // field is one of no byte), so nothing here reads a row end again
    uint32_t fields = 0;
    for (uint32_t c = 0; c < job.ncols; ++c) {
        const PbRowsJob col = cols[job.first_col + c];
        const uint32_t p = col_pay[col.first_row + r];
        fields += p + pb_records::FieldHeaderBytes(col.inner, col.kind, col.row_ends == nullptr, p);
    }
    const uint32_t hn = pb_records::RowHeaderBytes(job.number, fields);
    if ((uint64_t)off + hn + fields > total) return;  // nothing leaves the message
    pb_records::PutRowHeader(job.dst + off, job.number, fields);
    uint32_t at = off + hn;
    for (uint32_t c = 0; c < job.ncols; ++c) {
        const PbRowsJob col = cols[job.first_col + c];
        const uint32_t p = col_pay[col.first_row + r];
        at += pb_records::PutFieldHeader(job.dst + at, col.inner, col.kind, col.row_ends == nullptr, p);
        col_delta[col.first_row + r] = at - col_delta[col.first_row + r];
        at += p;
    }
}

__global__ void __launch_bounds__(kRunThreads) pb_records_place_kernel(
    const PbRecordsJob* __restrict__ jobs, const PbRowsJob* __restrict__ cols, int ncols,
    const uint32_t* __restrict__ groups, const uint32_t* __restrict__ block_off,
    const uint32_t* __restrict__ col_delta, const unsigned long long* __restrict__ bad,
    PbRecordsResult* __restrict__ res) {
    const PbRowsJob col = cols[wg::job_of<&PbRowsJob::first_chunk>(cols, ncols, blockIdx.x)];
    const int j = (int)col.first_rblock;  // a column's: its record job
    const PbRecordsJob job = jobs[j];
    if (bad[j] != kNoRecord) return;
    const uint32_t total = records_job_total(job, j, block_off);
    if (total > job.cap) return;
    rows_place_chunk<true>(col, blockIdx.x - col.first_chunk, total, groups, col_delta + col.first_row, &res[j].err);
}

// ------------------------------------------------------------ row splitter
// A message of rows -> the flat array and the row ends (kernels.h: init,
// spec, prefix, skip, chase, fill, mark, prefix, table, check, count, prefix,
// publish, ends, place; the wire rules are base/pb_rows.h).
constexpr uint32_t kSplitPer = kPbSplitChunk / kRunThreads;  // offsets per lane
constexpr uint32_t kSplitAhead = 32;                         // staged behind a chunk: >= pb_rows::kSpecReadBytes
constexpr uint32_t kSplitBack = 16;                          // staged in front of one: a varint's nine earlier bytes
constexpr int kSplitStage16 = (kSplitBack + kPbSplitChunk + kSplitAhead + 16 + 15) / 16;
static_assert(kPbSplitChunk == 64 * 64 && kRunThreads == 256 && kSplitAhead >= pb_rows::kSpecReadBytes, "split layout");
static_assert(2 * kRunThreads * 16 >= kSplitStage16 * 16, "two rounds of loads stage a chunk");

__device__ __forceinline__ uint64_t* split_row_table(const PbSplitJob& job, uint32_t* exit) {
    return reinterpret_cast<uint64_t*>(exit + (size_t)job.first_chunk * kPbSplitChunk);
}
// A row table entry: the tag's offset (28 bits), the bytes from there to the
// payload (6 bits: two tags and two lengths of ten bytes at most), the
// payload's bytes (28 bits).
__device__ __forceinline__ uint64_t split_row_pack(uint32_t tag_off, uint32_t head, uint32_t len) {
    return (uint64_t)tag_off | ((uint64_t)head << 28) | ((uint64_t)len << 34);
}
__device__ __forceinline__ uint32_t split_row_tag(uint64_t e) { return (uint32_t)e & 0x0FFFFFFFu; }
__device__ __forceinline__ uint32_t split_row_pay(uint64_t e) { return split_row_tag(e) + ((uint32_t)(e >> 28) & 63u); }
__device__ __forceinline__ uint32_t split_row_len(uint64_t e) { return (uint32_t)(e >> 34) & 0x0FFFFFFFu; }

__device__ __forceinline__ uint32_t split_total(const uint32_t* scanned, uint32_t first, uint32_t n) {
    return scanned[first + n] - scanned[first];
}

// Bytes without a continuation bit in [0, x) of the job's message, x <= n.
__device__ __forceinline__ uint32_t split_terms_before(const PbSplitJob& job, const uint64_t* term_mask,
                                                       const uint32_t* term_group, const uint32_t* term_chunk,
                                                       uint32_t x) {
    const uint32_t c = x / kPbSplitChunk;
    if (c >= job.nchunks) return split_total(term_chunk, job.first_chunk, job.nchunks);
    const size_t g = (size_t)(job.first_chunk + c) * 64 + ((x >> 6) & 63);
    return term_chunk[job.first_chunk + c] - term_chunk[job.first_chunk] + term_group[g] +
           (uint32_t)__popcll(term_mask[g] & ((1ull << (x & 63)) - 1));
}

__global__ void __launch_bounds__(64) pb_split_init_kernel(const PbSplitJob* __restrict__ jobs, int njobs,
                                                           PbSplitJob* __restrict__ jobs_dev,
                                                           uint32_t* __restrict__ term_chunk,
                                                           uint32_t* __restrict__ row_chunk,
                                                           uint32_t* __restrict__ block_sum, uint32_t nchunks,
                                                           uint32_t nrblocks, uint32_t* __restrict__ bad,
                                                           uint32_t* __restrict__ others, int32_t* __restrict__ ok) {
    const int j = (int)(blockIdx.x * 64 + threadIdx.x);
    if (j == 0) {
        // the entries behind the last job's, whose prefix is its total
        term_chunk[nchunks] = 0;
        row_chunk[nchunks] = 0;
        block_sum[nrblocks] = 0;
    }
    if (j >= njobs) return;
    jobs_dev[j] = jobs[j];
    bad[j] = kPbSplitNone;
    others[j] = 0;
    ok[j] = 0;
}

// Stages chunk bytes [-back, len + ahead) that lie inside the message and
// returns the LDS address of chunk byte 0.
__device__ __forceinline__ const uint8_t* split_stage(const PbSplitJob& job, uint32_t cs, uint32_t len, uint32_t back,
                                                      u32x4* lds) {
    back = back < cs ? back : cs;
    const uint32_t rest = job.n - cs;
    const uint32_t fwd = rest < len + kSplitAhead ? rest : len + kSplitAhead;
    const uint32_t a = wg::stage16<kRunThreads, 2>(job.msg + cs - back, back + fwd, lds);
    return reinterpret_cast<const uint8_t*>(lds) + a + back;
}

// next[] of every offset of the chunk: where the field that would start
// there ends, or none.
__device__ __forceinline__ void split_parse(const PbSplitJob& job, const uint8_t* bytes, uint32_t cs, uint32_t len,
                                            uint32_t* nxt) {
#pragma unroll 4
    for (uint32_t r = 0; r < kSplitPer; ++r) {
        const uint32_t i = r * kRunThreads + threadIdx.x;
        if (i >= len) continue;
        const pb_rows::Field f = pb_rows::SpecFieldAt(bytes + i, cs + i, job.n);
        nxt[i] = f.valid ? (uint32_t)f.next : kPbSplitNone;
    }
}

// Pointer doubling over the chunk's offsets: afterwards at[i] is the first
// offset on i's chain that is at or beyond the end of i's span (the chunk
// when span_shift is 12, its 64-byte sub-chunk when 6), or none. A chain
// grows by two bytes a hop at least, so a span of 2^k bytes is resolved
// after k - 1 rounds and the round that sees nothing move; reading an entry
// another lane has already advanced only gets there sooner.
__device__ __forceinline__ void split_resolve(uint32_t* at, uint32_t cs, uint32_t len, uint32_t span_shift) {
    for (uint32_t round = 0; round <= span_shift; ++round) {
        int moved = 0;
        for (uint32_t r = 0; r < kSplitPer; ++r) {
            const uint32_t i = r * kRunThreads + threadIdx.x;
            if (i >= len) continue;
            const uint32_t e = at[i];
            if (e == kPbSplitNone) continue;
            const uint32_t k = e - cs;  // > i
            if (k < len && (k >> span_shift) == (i >> span_shift)) {
                at[i] = at[k];
                moved = 1;
            }
        }
        if (!__syncthreads_or(moved)) break;
    }
}

__global__ void __launch_bounds__(kRunThreads) pb_split_spec_kernel(const PbSplitJob* __restrict__ jobs, int njobs,
                                                                    uint32_t* __restrict__ exit,
                                                                    uint64_t* __restrict__ term_mask,
                                                                    uint32_t* __restrict__ term_group,
                                                                    uint32_t* __restrict__ term_chunk,
                                                                    uint32_t* __restrict__ entry,
                                                                    uint32_t* __restrict__ land) {
    __shared__ u32x4 raw[kSplitStage16];
    __shared__ uint32_t nxt[kPbSplitChunk];
    __shared__ uint64_t groups[64];
    const PbSplitJob job = jobs[wg::job_of<&PbSplitJob::first_chunk>(jobs, njobs, blockIdx.x)];
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t cs = (blockIdx.x - job.first_chunk) * kPbSplitChunk;
    const uint32_t len = job.n - cs < kPbSplitChunk ? job.n - cs : kPbSplitChunk;
    const uint8_t* bytes = split_stage(job, cs, len, 0, raw);
    if (t == 0) {
        entry[blockIdx.x] = kPbSplitNone;
        if (land) land[blockIdx.x] = kPbSplitNone;
    }
    __syncthreads();
    split_parse(job, bytes, cs, len, nxt);
    // a wave's 64 bytes of a round are one group of the terminator mask
    for (uint32_t r = 0; r < kSplitPer; ++r) {
        const uint32_t i = r * kRunThreads + t;
        const uint64_t m = __ballot(i < len && !(bytes[i] & 0x80));
        if (lane == 0) groups[r * (kRunThreads / 64) + wave] = m;
    }
    __syncthreads();
    if (wave == 0) {
        const uint64_t m = groups[lane];
        const uint32_t mine = (uint32_t)__popcll(m);
        const uint32_t incl = wg::wave_incl_scan(mine);
        const size_t g = (size_t)blockIdx.x * 64 + lane;
        term_mask[g] = m;
        term_group[g] = incl - mine;
        if (lane == 63) term_chunk[blockIdx.x] = incl;
    }
    split_resolve(nxt, cs, len, 12);
    uint32_t* out = exit + (size_t)blockIdx.x * kPbSplitChunk;
    for (uint32_t r = 0; r < kSplitPer; ++r) {
        const uint32_t i = r * kRunThreads + t;
        if (i < len) out[i] = nxt[i];
    }
}

// skip[p] = exit applied `hops` times to p (none and n stay): what the chase
// follows, so that its serial hops are `hops` chunks long at least. Chains
// merge within a few fields, so the lanes of a wave mostly ask for the same
// few entries.
__global__ void __launch_bounds__(kRunThreads) pb_split_skip_kernel(const PbSplitJob* __restrict__ jobs, int njobs,
                                                                    const uint32_t* __restrict__ exit,
                                                                    uint32_t* __restrict__ skip, uint32_t hops) {
    const PbSplitJob job = jobs[wg::job_of<&PbSplitJob::first_chunk>(jobs, njobs, blockIdx.x)];
    const uint32_t cs = (blockIdx.x - job.first_chunk) * kPbSplitChunk;
    const uint32_t len = job.n - cs < kPbSplitChunk ? job.n - cs : kPbSplitChunk;
    const uint32_t* ex = exit + (size_t)job.first_chunk * kPbSplitChunk;
    uint32_t e[kSplitPer];
#pragma unroll
    for (uint32_t r = 0; r < kSplitPer; ++r) {
        const uint32_t i = r * kRunThreads + threadIdx.x;
        e[r] = i < len ? ex[cs + i] : kPbSplitNone;
    }
    for (uint32_t h = 1; h < hops; ++h) {
#pragma unroll
        for (uint32_t r = 0; r < kSplitPer; ++r) {
            if (e[r] < job.n) e[r] = ex[e[r]];  // none is above every n
        }
    }
    uint32_t* out = skip + (size_t)blockIdx.x * kPbSplitChunk;
#pragma unroll
    for (uint32_t r = 0; r < kSplitPer; ++r) {
        const uint32_t i = r * kRunThreads + threadIdx.x;
        if (i < len) out[i] = e[r];
    }
}

// `table` is exit[] (then `first` is entry[]) or skip[] (then `first` is
// land[], which the fill pass spreads into entry[]).
__global__ void __launch_bounds__(64) pb_split_chase_kernel(const PbSplitJob* __restrict__ jobs, int njobs,
                                                            const uint32_t* __restrict__ table,
                                                            uint32_t* __restrict__ first) {
    const int j = (int)(blockIdx.x * 64 + threadIdx.x);
    if (j >= njobs) return;
    const PbSplitJob job = jobs[j];
    const uint32_t* hop_to = table + (size_t)job.first_chunk * kPbSplitChunk;
    uint32_t pos = 0;
    // every hop lands in a later chunk
    for (uint32_t hop = 0; hop < job.nchunks && pos < job.n; ++hop) {
        first[job.first_chunk + pos / kPbSplitChunk] = pos;
        pos = hop_to[pos];  // none is above every n
    }
}

// A lane per chunk the chase landed in: the entries of the chunks between
// this landing and the next, `hops` - 1 hops of exit[] further.
__global__ void __launch_bounds__(64) pb_split_fill_kernel(const PbSplitJob* __restrict__ jobs, int njobs,
                                                           const uint32_t* __restrict__ exit,
                                                           const uint32_t* __restrict__ land,
                                                           uint32_t* __restrict__ entry, uint32_t hops,
                                                           uint32_t nchunks) {
    const uint32_t c = blockIdx.x * 64 + threadIdx.x;
    if (c >= nchunks) return;
    const PbSplitJob job = jobs[wg::job_of<&PbSplitJob::first_chunk>(jobs, njobs, c)];
    const uint32_t* ex = exit + (size_t)job.first_chunk * kPbSplitChunk;
    uint32_t pos = land[c];
    for (uint32_t h = 0; h < hops && pos < job.n; ++h) {
        entry[job.first_chunk + pos / kPbSplitChunk] = pos;
        pos = ex[pos];
    }
}

__global__ void __launch_bounds__(kRunThreads) pb_split_mark_kernel(const PbSplitJob* __restrict__ jobs, int njobs,
                                                                    const uint32_t* __restrict__ entry,
                                                                    uint64_t* __restrict__ row_mask,
                                                                    uint32_t* __restrict__ row_chunk,
                                                                    uint32_t* __restrict__ bad,
                                                                    uint32_t* __restrict__ others) {
    __shared__ u32x4 raw[kSplitStage16];
    __shared__ uint32_t nxt[kPbSplitChunk];
    __shared__ uint32_t sub[kPbSplitChunk];
    __shared__ uint32_t sub_entry[64];
    __shared__ uint64_t starts[64];
    __shared__ uint16_t row_bits[kRunThreads];  // lane t: its 16 offsets; four lanes make a group's mask
    __shared__ uint32_t tally[2];
    const int j = wg::job_of<&PbSplitJob::first_chunk>(jobs, njobs, blockIdx.x);
    const PbSplitJob job = jobs[j];
    const uint32_t t = threadIdx.x;
    const uint32_t ent = entry[blockIdx.x];
    if (ent == kPbSplitNone) {  // the walk jumped over this chunk, or ended before it
        if (t < 64) row_mask[(size_t)blockIdx.x * 64 + t] = 0;
        if (t == 0) row_chunk[blockIdx.x] = 0;
        return;
    }
    const uint32_t cs = (blockIdx.x - job.first_chunk) * kPbSplitChunk;
    const uint32_t len = job.n - cs < kPbSplitChunk ? job.n - cs : kPbSplitChunk;
    const uint8_t* bytes = split_stage(job, cs, len, 0, raw);
    if (t < 64) sub_entry[t] = kPbSplitNone;
    if (t < 2) tally[t] = 0;
    __syncthreads();
    split_parse(job, bytes, cs, len, nxt);
    for (uint32_t r = 0; r < kSplitPer; ++r) {
        const uint32_t i = r * kRunThreads + t;
        if (i < len) sub[i] = nxt[i];
    }
    __syncthreads();
    split_resolve(sub, cs, len, 6);
    if (t == 0) {
        // across the sub-chunks: every hop lands in a later one
        uint32_t pos = ent;
        for (uint32_t hop = 0; hop < 64 && pos != kPbSplitNone && pos - cs < len; ++hop) {
            sub_entry[(pos - cs) >> 6] = pos;
            pos = sub[pos - cs];
        }
    }
    __syncthreads();
    if (t < 64) {
        // inside one: at most 32 fields; an offset that is no field is still a
        // true start (the offender), and ends the walk
        uint64_t m = 0;
        uint32_t pos = sub_entry[t];
        for (uint32_t hop = 0; hop < 32 && pos != kPbSplitNone && pos - cs < len && ((pos - cs) >> 6) == t; ++hop) {
            m |= 1ull << ((pos - cs) & 63);
            pos = nxt[pos - cs];
        }
        starts[t] = m;
    }
    __syncthreads();
    uint32_t mine = (uint32_t)(starts[t >> 2] >> ((t & 3) * 16)) & 0xFFFFu, rows = 0, nrows = 0, nothers = 0;
    while (mine) {
        const uint32_t bit = (uint32_t)__ffs((int)mine) - 1;
        mine &= mine - 1;
        const uint32_t i = t * 16 + bit;
        const pb_rows::Field f = pb_rows::SpecFieldAt(bytes + i, cs + i, job.n);
        if (!f.valid) {
            atomicMin(&bad[j], ((cs + i) << 3) | (uint32_t)pb_rows::kSplitMalformed);
        } else if ((f.tag >> 3) != job.number) {
            ++nothers;
        } else if ((f.tag & 7) != 2) {
            atomicMin(&bad[j], ((cs + i) << 3) | (uint32_t)pb_rows::kSplitUnsupported);
        } else {
            rows |= 1u << bit;
            ++nrows;
        }
    }
    row_bits[t] = (uint16_t)rows;
    nrows = wg::wave_sum(nrows);
    nothers = wg::wave_sum(nothers);
    if ((t & 63) == 0) {
        atomicAdd(&tally[0], nrows);
        atomicAdd(&tally[1], nothers);
    }
    __syncthreads();
    if (t < 64) {
        const uint64_t m = (uint64_t)row_bits[4 * t] | ((uint64_t)row_bits[4 * t + 1] << 16) |
                           ((uint64_t)row_bits[4 * t + 2] << 32) | ((uint64_t)row_bits[4 * t + 3] << 48);
        row_mask[(size_t)blockIdx.x * 64 + t] = m;
    }
    if (t == 0) {
        row_chunk[blockIdx.x] = tally[0];
        if (tally[1]) atomicAdd(&others[j], tally[1]);
    }
}

__global__ void __launch_bounds__(kRunThreads) pb_split_table_kernel(const PbSplitJob* __restrict__ jobs, int njobs,
                                                                     const uint64_t* __restrict__ row_mask,
                                                                     const uint32_t* __restrict__ row_chunk,
                                                                     uint32_t* __restrict__ exit,
                                                                     uint32_t* __restrict__ bad) {
    __shared__ uint32_t before[64];
    const int j = wg::job_of<&PbSplitJob::first_chunk>(jobs, njobs, blockIdx.x);
    const PbSplitJob job = jobs[j];
    if (row_chunk[blockIdx.x + 1] == row_chunk[blockIdx.x]) return;
    const uint32_t t = threadIdx.x, lane = t & 63;
    const uint32_t cs = (blockIdx.x - job.first_chunk) * kPbSplitChunk;
    if (t < 64) {
        const uint32_t mine = (uint32_t)__popcll(row_mask[(size_t)blockIdx.x * 64 + t]);
        before[t] = wg::wave_incl_scan(mine) - mine;
    }
    __syncthreads();
    const uint64_t m = row_mask[(size_t)blockIdx.x * 64 + (t >> 2)];
    const uint32_t sh = (t & 3) * 16;
    uint32_t mine = (uint32_t)(m >> sh) & 0xFFFFu;
    // rows of the job in front of this lane's: at most n / 2 rows, so the
    // table stays inside the job's part of exit[]
    uint32_t rank = row_chunk[blockIdx.x] - row_chunk[job.first_chunk] + before[t >> 2] +
                    (uint32_t)__popcll(m & ((1ull << sh) - 1));
    uint64_t* table = split_row_table(job, exit);
    while (mine) {
        const uint32_t bit = (uint32_t)__ffs((int)mine) - 1;
        mine &= mine - 1;
        const uint32_t p = cs + t * 16 + bit;
        const pb_rows::Field f = pb_rows::SpecField(job.msg, p, job.n);  // a row: the mark pass parsed it
        uint64_t po = 0, pl = 0;
        const int code = f.valid ? pb_rows::RowShape(job.msg, f.vpos, f.vlen, job.inner, job.kind, &po, &pl)
                                 : pb_rows::kSplitMalformed;
        if (code != 0) {
            atomicMin(&bad[j], (p << 3) | (uint32_t)code);
            po = p;
            pl = 0;
        }
        if ((uint64_t)rank < job.n / 2 + 1) table[rank] = split_row_pack(p, (uint32_t)(po - p), (uint32_t)pl);
        ++rank;
    }
}

// The row whose payload holds byte q, among rows [lo, hi) of the table, or
// none: the last one whose payload starts at or before q, if q is inside it.
__device__ __forceinline__ uint32_t split_row_of(const uint64_t* table, uint32_t lo, uint32_t hi, uint32_t q,
                                                 uint64_t* entry) {
    if (lo >= hi || split_row_pay(table[lo]) > q) return kPbSplitNone;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (split_row_pay(table[mid]) <= q) {
            lo = mid;
        } else {
            hi = mid;
        }
    }
    const uint64_t e = table[lo];
    *entry = e;
    return q - split_row_pay(e) < split_row_len(e) ? lo : kPbSplitNone;
}

// Varint kinds, a workgroup per message chunk. kPlace false: the check pass
// (a varint the packed-run decoder refuses, inside a payload, is reported).
// kPlace true: the place pass (every terminator inside a payload ends one
// element). A varint's extent needs no row bounds: the byte in front of a
// payload is the last of a length, so it has no continuation bit.
template <bool kPlace>
__global__ void __launch_bounds__(kRunThreads) pb_split_varint_kernel(const PbSplitJob* __restrict__ jobs, int njobs,
                                                                      const uint32_t* __restrict__ exit,
                                                                      const uint64_t* __restrict__ term_mask,
                                                                      const uint32_t* __restrict__ term_group,
                                                                      const uint32_t* __restrict__ term_chunk,
                                                                      const uint32_t* __restrict__ row_chunk,
                                                                      const uint32_t* __restrict__ row_bias,
                                                                      uint32_t* __restrict__ bad,
                                                                      const int32_t* __restrict__ ok) {
    __shared__ u32x4 raw[kSplitStage16];
    const int j = wg::job_of<&PbSplitJob::first_chunk>(jobs, njobs, blockIdx.x);
    const PbSplitJob job = jobs[j];
    if (!pb_rows::WireIsVarint(job.kind) || (kPlace && !ok[j])) return;
    // the rows that start in this chunk, and the one before them that may reach into it
    const uint32_t first = row_chunk[job.first_chunk];
    const uint32_t hi = row_chunk[blockIdx.x + 1] - first;
    uint32_t lo = row_chunk[blockIdx.x] - first;
    lo = lo ? lo - 1 : 0;
    if (lo >= hi) return;
    const uint32_t t = threadIdx.x;
    const uint32_t cs = (blockIdx.x - job.first_chunk) * kPbSplitChunk;
    const uint32_t len = job.n - cs < kPbSplitChunk ? job.n - cs : kPbSplitChunk;
    const uint8_t* bytes = split_stage(job, cs, len, kSplitBack, raw);
    const uint64_t* table = split_row_table(job, const_cast<uint32_t*>(exit));
    const size_t g = (size_t)blockIdx.x * 64 + (t >> 2);
    const uint64_t m = term_mask[g];
    uint32_t terms = 0;  // terminators in front of this lane's bytes
    if (kPlace) {
        terms = term_chunk[blockIdx.x] - term_chunk[job.first_chunk] + term_group[g] +
                (uint32_t)__popcll(m & ((1ull << ((t & 3) * 16)) - 1));
    }
    __syncthreads();
    uint32_t mine = (uint32_t)(m >> ((t & 3) * 16)) & 0xFFFFu;
    while (mine) {
        const uint32_t bit = (uint32_t)__ffs((int)mine) - 1;
        mine &= mine - 1;
        const int i = (int)(t * 16 + bit);  // bytes[i - 10 ..] is staged when it is in the message
        const uint32_t q = cs + (uint32_t)i;
        uint32_t nb = 1;  // bytes of the varint that ends at q; 11: more than ten
        uint64_t v = bytes[i] & 0x7f;
        while (nb <= 10 && nb <= q && (bytes[i - (int)nb] & 0x80)) {
            v = (v << 7) | (bytes[i - (int)nb] & 0x7f);
            ++nb;
        }
        const bool refused = nb > 10 || (nb == 10 && bytes[i] > 1);
        if (kPlace || refused) {
            uint64_t e = 0;
            const uint32_t r = split_row_of(table, lo, hi, q, &e);
            if (r != kPbSplitNone) {
                if (!kPlace) {
                    atomicMin(&bad[j], (split_row_tag(e) << 3) | (uint32_t)pb_rows::kSplitMalformed);
                } else {
                    const uint32_t at = row_bias[job.first_row + r] + terms;
                    if ((uint64_t)at < job.cap) pb_rows::StoreVarintElem(job.values, at, job.kind, v);
                }
            }
        }
        ++terms;
    }
}

// A lane per row, 256 rows to a workgroup. kEnds false: the count pass (the
// elements of each block of rows). kEnds true: row_ends, and for varint
// kinds row_bias, of the jobs that passed.
template <bool kEnds>
__global__ void __launch_bounds__(kPbSplitBlockRows) pb_split_rows_kernel(const PbSplitJob* __restrict__ jobs,
                                                                          int njobs,
                                                                          const uint32_t* __restrict__ exit,
                                                                          const uint64_t* __restrict__ term_mask,
                                                                          const uint32_t* __restrict__ term_group,
                                                                          const uint32_t* __restrict__ term_chunk,
                                                                          const uint32_t* __restrict__ row_chunk,
                                                                          uint32_t* __restrict__ block_sum,
                                                                          uint32_t* __restrict__ row_bias,
                                                                          const int32_t* __restrict__ ok) {
    __shared__ uint32_t wave_tot[kPbSplitBlockRows / 64];
    const int j = wg::job_of<&PbSplitJob::first_rblock>(jobs, njobs, blockIdx.x);
    const PbSplitJob job = jobs[j];
    if (kEnds && !ok[j]) return;
    const uint32_t rows = split_total(row_chunk, job.first_chunk, job.nchunks);
    const uint32_t r = (blockIdx.x - job.first_rblock) * kPbSplitBlockRows + threadIdx.x;
    const bool varints = pb_rows::WireIsVarint(job.kind);
    uint32_t ne = 0, front = 0;
    if (r < rows) {
        const uint64_t e = split_row_table(job, const_cast<uint32_t*>(exit))[r];
        const uint32_t po = split_row_pay(e), pl = split_row_len(e);
        if (varints) {
            front = split_terms_before(job, term_mask, term_group, term_chunk, po);
            ne = split_terms_before(job, term_mask, term_group, term_chunk, po + pl) - front;
        } else {
            ne = pl / pb_rows::SourceBytes(job.kind);
        }
    }
    uint32_t sum;
    uint32_t before = wg::block_excl_scan<(int)kPbSplitBlockRows>(ne, wave_tot, &sum);
    if (!kEnds) {
        if (threadIdx.x == 0) block_sum[blockIdx.x] = sum;
        return;
    }
    if (r >= rows) return;  // rows <= row_cap, count <= cap: the job passed
    before += block_sum[blockIdx.x] - block_sum[job.first_rblock];
    job.row_ends[r] = before + ne;
    if (varints) row_bias[job.first_row + r] = before - front;
}

__global__ void __launch_bounds__(64) pb_split_publish_kernel(const PbSplitJob* __restrict__ jobs, int njobs,
                                                              const uint32_t* __restrict__ row_chunk,
                                                              const uint32_t* __restrict__ block_sum,
                                                              const uint32_t* __restrict__ bad,
                                                              const uint32_t* __restrict__ others,
                                                              int32_t* __restrict__ ok,
                                                              PbSplitResult* __restrict__ res) {
    const int j = (int)(blockIdx.x * 64 + threadIdx.x);
    if (j >= njobs) return;
    const PbSplitJob job = jobs[j];
    const uint32_t key = bad[j];
    PbSplitResult out = {0, 0, 0, kPbSplitNone, 0};
    if (key != kPbSplitNone) {
        out.first_bad = key >> 3;
        out.err = (int32_t)(key & 7);
    } else {
        out.count = split_total(block_sum, job.first_rblock, job.nrblocks);
        out.rows = split_total(row_chunk, job.first_chunk, job.nchunks);
        out.others = others[j];
        if (out.count > job.cap || out.rows > job.row_cap) out.err = pb_rows::kSplitShort;
    }
    ok[j] = out.err == 0;
    res[j] = out;
}

// Fixed-width kinds and bytes: a workgroup per 2048 elements of the output.
__global__ void __launch_bounds__(kRunThreads) pb_split_place_kernel(const PbSplitJob* __restrict__ jobs, int njobs,
                                                                     const uint32_t* __restrict__ exit,
                                                                     const uint32_t* __restrict__ row_chunk,
                                                                     const uint32_t* __restrict__ block_sum,
                                                                     const int32_t* __restrict__ ok) {
    const int j = wg::job_of<&PbSplitJob::first_ochunk>(jobs, njobs, blockIdx.x);
    const PbSplitJob job = jobs[j];
    if (!ok[j]) return;
    const uint32_t count = split_total(block_sum, job.first_rblock, job.nrblocks);
    const uint32_t rows = split_total(row_chunk, job.first_chunk, job.nchunks);
    const uint32_t i0 = (blockIdx.x - job.first_ochunk) * kPbSplitOutChunk;
    if (i0 >= count || rows == 0) return;
    const uint32_t i1 = count - i0 < kPbSplitOutChunk ? count - 1 : i0 + kPbSplitOutChunk - 1;
    const uint32_t* ends = job.row_ends;
    // the first row whose end lies beyond element i, among rows [lo, hi]
    auto row_of = [ends](uint32_t lo, uint32_t hi, uint32_t i) {
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (ends[mid] > i) {
                hi = mid;
            } else {
                lo = mid + 1;
            }
        }
        return lo;
    };
    const uint32_t r_lo = row_of(0, rows - 1, i0), r_hi = row_of(r_lo, rows - 1, i1);
    const uint64_t* table = split_row_table(job, const_cast<uint32_t*>(exit));
    const uint32_t w = pb_rows::SourceBytes(job.kind);
    for (uint32_t k = 0; k < kPbSplitOutChunk / kRunThreads; ++k) {
        const uint32_t i = i0 + k * kRunThreads + threadIdx.x;
        if (i > i1) break;
        const uint32_t r = row_of(r_lo, r_hi, i);
        const uint32_t start = r ? ends[r - 1] : 0;
        const uint64_t e = table[r];
        const uint32_t off = (i - start) * w;
        if (i < start || off + w > split_row_len(e)) continue;  // never: row_ends are sums of these lengths
        const uint8_t* s = job.msg + split_row_pay(e) + off;
        uint64_t v = 0;
        for (uint32_t b = 0; b < w; ++b) v |= (uint64_t)s[b] << (8 * b);
        if (w == 1) {
            static_cast<uint8_t*>(job.values)[i] = (uint8_t)v;
        } else if (w == 4) {
            static_cast<uint32_t*>(job.values)[i] = (uint32_t)v;
        } else {
            static_cast<uint64_t*>(job.values)[i] = v;
        }
    }
}


// ---------------------------------------------------------- record splitter
// A message of records -> every column's flat array, row ends and scalars
// (kernels.h: the row splitter's passes up to the row ranks, then init, table,
// check, count, prefix, publish, ends, place; the rules are
// base/pb_records.h). A table entry is the payload's offset (28 bits), its
// bytes (28 bits) and a taken bit; an untaken one is 0, a payload of no byte.
constexpr uint64_t kRecTaken = 1ull << 56;
__device__ __forceinline__ uint64_t rec_pack(uint32_t off, uint32_t len) {
    return (uint64_t)off | ((uint64_t)len << 28) | kRecTaken;
}
__device__ __forceinline__ bool rec_taken(uint64_t e) { return (e & kRecTaken) != 0; }
__device__ __forceinline__ uint32_t rec_off(uint64_t e) { return (uint32_t)e & 0x0FFFFFFFu; }
__device__ __forceinline__ uint32_t rec_len(uint64_t e) { return (uint32_t)(e >> 28) & 0x0FFFFFFFu; }

__global__ void __launch_bounds__(64) pb_recsplit_init_kernel(const PbRecSplitJob* __restrict__ jobs, int njobs,
                                                              PbRecSplitJob* __restrict__ jobs_dev,
                                                              const PbRecSplitCol* __restrict__ cols, int ncols,
                                                              PbRecSplitCol* __restrict__ cols_dev,
                                                              pb_records::SplitColumn* __restrict__ specs,
                                                              uint32_t* __restrict__ absent,
                                                              uint32_t* __restrict__ block_sum, uint32_t nbsums) {
    const int i = (int)(blockIdx.x * 64 + threadIdx.x);
    if (i == 0) block_sum[nbsums] = 0;  // behind the last column's: its prefix is that column's total
    if (i < njobs) jobs_dev[i] = jobs[i];
    if (i >= ncols) return;
    const PbRecSplitCol col = cols[i];
    cols_dev[i] = col;
    specs[i].inner = col.inner;
    specs[i].kind = col.kind;
    specs[i].scalar = col.scalar;
    absent[i] = 0;
}

__global__ void __launch_bounds__(kRunThreads) pb_recsplit_table_kernel(
    const PbSplitJob* __restrict__ jobs, int njobs, const PbRecSplitJob* __restrict__ rjobs,
    const pb_records::SplitColumn* __restrict__ specs, const uint64_t* __restrict__ row_mask,
    const uint32_t* __restrict__ row_chunk, uint64_t* __restrict__ entry, uint32_t* __restrict__ rec_tag,
    uint32_t* __restrict__ bad) {
    __shared__ uint32_t before[64];
    const int j = wg::job_of<&PbSplitJob::first_chunk>(jobs, njobs, blockIdx.x);
    const PbSplitJob job = jobs[j];
    const PbRecSplitJob rj = rjobs[j];
    if (row_chunk[blockIdx.x + 1] == row_chunk[blockIdx.x]) return;
    const uint32_t t = threadIdx.x;
    const uint32_t cs = (blockIdx.x - job.first_chunk) * kPbSplitChunk;
    if (t < 64) {
        const uint32_t mine = (uint32_t)__popcll(row_mask[(size_t)blockIdx.x * 64 + t]);
        before[t] = wg::wave_incl_scan(mine) - mine;
    }
    __syncthreads();
    const uint64_t m = row_mask[(size_t)blockIdx.x * 64 + (t >> 2)];
    const uint32_t sh = (t & 3) * 16;
    uint32_t mine = (uint32_t)(m >> sh) & 0xFFFFu;
    uint32_t rank = row_chunk[blockIdx.x] - row_chunk[job.first_chunk] + before[t >> 2] +
                    (uint32_t)__popcll(m & ((1ull << sh) - 1));
    const pb_records::SplitColumn* cols = specs + rj.first_col;
    while (mine) {
        const uint32_t bit = (uint32_t)__ffs((int)mine) - 1;
        mine &= mine - 1;
        const uint32_t p = cs + t * 16 + bit;
        const pb_rows::Field f = pb_rows::SpecField(job.msg, p, job.n);  // a record: the mark pass parsed it
        // a record beyond the table is judged all the same: 1 and 6 win over 5
        const bool keep = rank < rj.rec_cap;
        uint64_t* row = entry + rj.first_entry + (uint64_t)rank * rj.ncols;
        if (keep) {
            rec_tag[rj.first_tag + rank] = p;
            for (uint32_t c = 0; c < rj.ncols; ++c) row[c] = 0;
        }
        int code = pb_rows::kSplitMalformed;
        if (f.valid) {
            bool refused = false;
            code = pb_records::RecordShape(job.msg, f.vpos, f.vlen, cols, rj.ncols,
                                           [&](uint32_t c, uint64_t off, uint64_t len) {
                                               if (keep) {
                                                   row[c] = rec_pack((uint32_t)off, (uint32_t)len);
                                               } else if (!cols[c].scalar && pb_rows::WireIsVarint(cols[c].kind)) {
                                                   uint64_t ne = 0;  // the check pass cannot find this record
                                                   if (!pb_rows::VarintsOk(job.msg + off, len, &ne)) refused = true;
                                               }
                                           });
            if (refused) code = pb_rows::kSplitMalformed;
        }
        if (code != 0) atomicMin(&bad[j], (p << 3) | (uint32_t)code);
        ++rank;
    }
}

// Ragged varint columns, a workgroup per message chunk. kPlace false: the
// check pass (a varint the packed-run decoder refuses, inside a taken varint
// payload, is reported). kPlace true: the place pass (every terminator inside
// such a payload ends one element).
template <bool kPlace>
__global__ void __launch_bounds__(kRunThreads) pb_recsplit_varint_kernel(
    const PbSplitJob* __restrict__ jobs, int njobs, const PbRecSplitJob* __restrict__ rjobs,
    const PbRecSplitCol* __restrict__ cols, const uint64_t* __restrict__ entry, const uint32_t* __restrict__ rec_tag,
    const uint32_t* __restrict__ bias, const uint64_t* __restrict__ term_mask, const uint32_t* __restrict__ term_group,
    const uint32_t* __restrict__ term_chunk, const uint32_t* __restrict__ row_chunk, uint32_t* __restrict__ bad,
    const int32_t* __restrict__ ok) {
    __shared__ u32x4 raw[kSplitStage16];
    const int j = wg::job_of<&PbSplitJob::first_chunk>(jobs, njobs, blockIdx.x);
    const PbSplitJob job = jobs[j];
    const PbRecSplitJob rj = rjobs[j];
    if (!rj.any_varint || (kPlace && !ok[j])) return;
    // the records that start in this chunk, and the one before them that may reach into it
    const uint32_t first = row_chunk[job.first_chunk];
    uint32_t hi = row_chunk[blockIdx.x + 1] - first;
    uint32_t lo = row_chunk[blockIdx.x] - first;
    lo = lo ? lo - 1 : 0;
    if (hi > rj.rec_cap) hi = rj.rec_cap;  // the table pass checked the records beyond the table itself
    if (lo >= hi) return;
    const uint32_t t = threadIdx.x;
    const uint32_t cs = (blockIdx.x - job.first_chunk) * kPbSplitChunk;
    const uint32_t len = job.n - cs < kPbSplitChunk ? job.n - cs : kPbSplitChunk;
    const uint8_t* bytes = split_stage(job, cs, len, kSplitBack, raw);
    const uint32_t* tags = rec_tag + rj.first_tag;
    const size_t g = (size_t)blockIdx.x * 64 + (t >> 2);
    const uint64_t m = term_mask[g];
    uint32_t terms = 0;  // terminators in front of this lane's bytes
    if (kPlace) {
        terms = term_chunk[blockIdx.x] - term_chunk[job.first_chunk] + term_group[g] +
                (uint32_t)__popcll(m & ((1ull << ((t & 3) * 16)) - 1));
    }
    __syncthreads();
    uint32_t mine = (uint32_t)(m >> ((t & 3) * 16)) & 0xFFFFu;
    while (mine) {
        const uint32_t bit = (uint32_t)__ffs((int)mine) - 1;
        mine &= mine - 1;
        const int i = (int)(t * 16 + bit);  // bytes[i - 10 ..] is staged when it is in the message
        const uint32_t q = cs + (uint32_t)i;
        uint32_t nb = 1;  // bytes of the varint that ends at q; 11: more than ten
        uint64_t v = bytes[i] & 0x7f;
        while (nb <= 10 && nb <= q && (bytes[i - (int)nb] & 0x80)) {
            v = (v << 7) | (bytes[i - (int)nb] & 0x7f);
            ++nb;
        }
        const bool refused = nb > 10 || (nb == 10 && bytes[i] > 1);
        if ((kPlace || refused) && tags[lo] <= q) {
            // the last record whose tag is at or before q, then the column whose payload holds q
            uint32_t a = lo, z = hi;
            while (z - a > 1) {
                const uint32_t mid = a + (z - a) / 2;
                if (tags[mid] <= q) {
                    a = mid;
                } else {
                    z = mid;
                }
            }
            const uint64_t at0 = rj.first_entry + (uint64_t)a * rj.ncols;
            for (uint32_t c = 0; c < rj.ncols; ++c) {
                const uint64_t e = entry[at0 + c];
                if (!rec_taken(e) || q - rec_off(e) >= rec_len(e)) continue;  // q below the offset wraps
                const PbRecSplitCol& col = cols[rj.first_col + c];
                if (col.scalar || !pb_rows::WireIsVarint(col.kind)) break;  // no element ends here
                if (!kPlace) {
                    atomicMin(&bad[j], (tags[a] << 3) | (uint32_t)pb_rows::kSplitMalformed);
                } else {
                    const uint32_t at = bias[at0 + c] + terms;
                    if ((uint64_t)at < col.cap) pb_rows::StoreVarintElem(col.values, at, col.kind, v);
                }
                break;
            }
        }
        ++terms;
    }
}

// A workgroup per 256 records, column after column. kEnds false: the count
// pass (each column's elements in the block, the absent scalars). kEnds true:
// row_ends, bias and the scalar values of the jobs that passed.
template <bool kEnds>
__global__ void __launch_bounds__(kPbSplitBlockRows) pb_recsplit_rows_kernel(
    const PbSplitJob* __restrict__ jobs, int njobs, const PbRecSplitJob* __restrict__ rjobs,
    const PbRecSplitCol* __restrict__ cols, const uint64_t* __restrict__ entry,
    const uint64_t* __restrict__ term_mask, const uint32_t* __restrict__ term_group,
    const uint32_t* __restrict__ term_chunk, const uint32_t* __restrict__ row_chunk, uint32_t* __restrict__ block_sum,
    uint32_t* __restrict__ bias, uint32_t* __restrict__ absent, const int32_t* __restrict__ ok) {
    __shared__ uint32_t wave_tot[kPbSplitBlockRows / 64];
    const int j = wg::job_of<&PbRecSplitJob::first_rblock>(rjobs, njobs, blockIdx.x);
    const PbSplitJob job = jobs[j];
    const PbRecSplitJob rj = rjobs[j];
    if (kEnds && !ok[j]) return;
    uint32_t rows = split_total(row_chunk, job.first_chunk, job.nchunks);
    if (rows > rj.rec_cap) rows = rj.rec_cap;  // the job ends with 5 (or 1, 6): its counts are not reported
    const uint32_t blk = blockIdx.x - rj.first_rblock;
    const uint32_t r = blk * kPbSplitBlockRows + threadIdx.x;
    for (uint32_t c = 0; c < rj.ncols; ++c) {
        const PbRecSplitCol col = cols[rj.first_col + c];
        const uint64_t at = rj.first_entry + (uint64_t)r * rj.ncols + c;
        const uint64_t e = r < rows ? entry[at] : 0;
        const bool varints = pb_rows::WireIsVarint(col.kind);
        if (col.scalar) {
            if (!kEnds) {
                const uint32_t miss = wg::wave_sum((uint32_t)(r < rows && !rec_taken(e)));
                if ((threadIdx.x & 63) == 0 && miss) atomicAdd(&absent[rj.first_col + c], miss);
                if (threadIdx.x == 0) block_sum[col.first_bsum + blk] = 0;  // its count is the records
            } else if (r < rows) {
                // r < rows <= cap: the job passed. An absent scalar reads as 0.
                const uint8_t* s = job.msg + rec_off(e);
                uint64_t v = 0;
                if (varints) {
                    uint32_t used = 0;
                    if (rec_taken(e)) pb_rows::GetVarint(s, rec_len(e), &used, &v);
                    pb_rows::StoreVarintElem(col.values, r, col.kind, v);
                } else {
                    const uint32_t w = pb_rows::SourceBytes(col.kind);
                    for (uint32_t b = 0; b < w && rec_taken(e); ++b) v |= (uint64_t)s[b] << (8 * b);
                    if (w == 4) {
                        static_cast<uint32_t*>(col.values)[r] = (uint32_t)v;
                    } else {
                        static_cast<uint64_t*>(col.values)[r] = v;
                    }
                }
            }
            continue;
        }
        uint32_t ne = 0, front = 0;
        if (r < rows) {
            const uint32_t po = rec_off(e), pl = rec_len(e);
            if (!varints) {
                ne = pl / pb_rows::SourceBytes(col.kind);
            } else if (pl > 0) {
                front = split_terms_before(job, term_mask, term_group, term_chunk, po);
                ne = split_terms_before(job, term_mask, term_group, term_chunk, po + pl) - front;
            }
        }
        uint32_t sum;
        uint32_t before = wg::block_excl_scan<(int)kPbSplitBlockRows>(ne, wave_tot, &sum);
        __syncthreads();  // the next column's scan writes wave_tot again
        if (!kEnds) {
            if (threadIdx.x == 0) block_sum[col.first_bsum + blk] = sum;
            continue;
        }
        if (r >= rows) continue;  // rows <= row_cap, count <= cap: the job passed
        before += block_sum[col.first_bsum + blk] - block_sum[col.first_bsum];
        col.row_ends[r] = before + ne;
        if (varints) bias[at] = before - front;
    }
}

__global__ void __launch_bounds__(64) pb_recsplit_publish_kernel(
    const PbSplitJob* __restrict__ jobs, int njobs, const PbRecSplitJob* __restrict__ rjobs,
    const PbRecSplitCol* __restrict__ cols, const uint32_t* __restrict__ row_chunk,
    const uint32_t* __restrict__ block_sum, const uint32_t* __restrict__ absent, const uint32_t* __restrict__ bad,
    const uint32_t* __restrict__ others, int32_t* __restrict__ ok, PbRecSplitResult* __restrict__ res) {
    const int j = (int)(blockIdx.x * 64 + threadIdx.x);
    if (j >= njobs) return;
    const PbSplitJob job = jobs[j];
    const PbRecSplitJob rj = rjobs[j];
    const uint32_t key = bad[j];
    // res[j] arrives zeroed, first_bad none: the counts of a job that fails with 1 or 6, or with more
    // records than row_cap, stay 0
    int32_t err = 0;
    if (key != kPbSplitNone) {
        res[j].first_bad = key >> 3;
        err = (int32_t)(key & 7);
    } else {
        const uint32_t rows = split_total(row_chunk, job.first_chunk, job.nchunks);
        res[j].rows = rows;
        res[j].others = others[j];
        if (rows > rj.row_cap) {
            err = pb_rows::kSplitShort;
        } else {
            for (uint32_t c = 0; c < rj.ncols; ++c) {
                const PbRecSplitCol& col = cols[rj.first_col + c];
                const uint64_t count = col.scalar ? rows : split_total(block_sum, col.first_bsum, rj.nrblocks);
                res[j].count[c] = count;
                res[j].absent[c] = col.scalar ? absent[rj.first_col + c] : 0;
                if (count > col.cap) err = pb_rows::kSplitShort;
            }
        }
    }
    res[j].err = err;
    ok[j] = err == 0;
}

// Ragged fixed-width and bytes columns: a workgroup per 2048 elements of one
// column's output.
__global__ void __launch_bounds__(kRunThreads) pb_recsplit_place_kernel(
    const PbSplitJob* __restrict__ jobs, const PbRecSplitJob* __restrict__ rjobs,
    const PbRecSplitCol* __restrict__ cols, int ncols, const uint64_t* __restrict__ entry,
    const uint32_t* __restrict__ row_chunk, const uint32_t* __restrict__ block_sum, const int32_t* __restrict__ ok) {
    const PbRecSplitCol col = cols[wg::job_of<&PbRecSplitCol::first_ochunk>(cols, ncols, blockIdx.x)];
    const int j = (int)col.job;
    if (!ok[j] || blockIdx.x - col.first_ochunk >= col.nochunks) return;
    const PbSplitJob job = jobs[j];
    const PbRecSplitJob rj = rjobs[j];
    const uint32_t count = split_total(block_sum, col.first_bsum, rj.nrblocks);
    const uint32_t rows = split_total(row_chunk, job.first_chunk, job.nchunks);
    const uint32_t i0 = (blockIdx.x - col.first_ochunk) * kPbSplitOutChunk;
    if (i0 >= count || rows == 0) return;
    const uint32_t i1 = count - i0 < kPbSplitOutChunk ? count - 1 : i0 + kPbSplitOutChunk - 1;
    const uint32_t* ends = col.row_ends;
    // the first record whose end lies beyond element i, among records [lo, hi]
    auto row_of = [ends](uint32_t lo, uint32_t hi, uint32_t i) {
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (ends[mid] > i) {
                hi = mid;
            } else {
                lo = mid + 1;
            }
        }
        return lo;
    };
    const uint32_t r_lo = row_of(0, rows - 1, i0), r_hi = row_of(r_lo, rows - 1, i1);
    const uint32_t w = pb_rows::SourceBytes(col.kind);
    for (uint32_t k = 0; k < kPbSplitOutChunk / kRunThreads; ++k) {
        const uint32_t i = i0 + k * kRunThreads + threadIdx.x;
        if (i > i1) break;
        const uint32_t r = row_of(r_lo, r_hi, i);
        const uint32_t start = r ? ends[r - 1] : 0;
        const uint64_t e = entry[rj.first_entry + (uint64_t)r * rj.ncols + col.index];
        const uint32_t off = (i - start) * w;
        if (i < start || off + w > rec_len(e)) continue;  // never: row_ends are sums of these lengths
        const uint8_t* s = job.msg + rec_off(e) + off;
        uint64_t v = 0;
        for (uint32_t b = 0; b < w; ++b) v |= (uint64_t)s[b] << (8 * b);
        if (w == 1) {
            static_cast<uint8_t*>(col.values)[i] = (uint8_t)v;
        } else if (w == 4) {
            static_cast<uint32_t*>(col.values)[i] = (uint32_t)v;
        } else {
            static_cast<uint64_t*>(col.values)[i] = v;
        }
    }
}

}  // namespace

#define SPLIT_LAUNCH(kernel, grid, block, ...)                          \
    hipLaunchKernelGGL(kernel, grid, block, 0, s, t.jobs_dev, t.njobs, __VA_ARGS__); \
    if (hipGetLastError() != hipSuccess) return -1

// The passes both splitters share: the top-level field starts, and with them
// every occurrence of `number` marked and ranked (row_chunk scanned).
static int split_front(const PbSplitTables& t, hipStream_t s) {
    if (!t.jobs || !t.jobs_dev || !t.exit || !t.term_mask || !t.row_mask || !t.term_group || !t.term_chunk ||
        !t.row_chunk || !t.entry || !t.block_sum || !t.bad || !t.others || !t.ok || t.nchunks == 0 ||
        t.nrblocks == 0 || t.nchunks > 0x7FFFFFFEu || t.nrblocks > 0x7FFFFFFEu || (t.nrows > 0 && !t.row_bias) ||
        t.skip_hops == 0 || (t.skip_hops > 1 && (!t.skip || !t.land))) {
        return -1;
    }
    const bool skips = t.skip_hops > 1;
    const dim3 per_job((unsigned)(t.njobs + 63) / 64), wave(64), wg(kRunThreads);
    hipLaunchKernelGGL(pb_split_init_kernel, per_job, wave, 0, s, t.jobs, t.njobs, t.jobs_dev, t.term_chunk,
                       t.row_chunk, t.block_sum, t.nchunks, t.nrblocks, t.bad, t.others, t.ok);
    if (hipGetLastError() != hipSuccess) return -1;
    SPLIT_LAUNCH(pb_split_spec_kernel, dim3(t.nchunks), wg, t.exit, t.term_mask, t.term_group, t.term_chunk, t.entry,
                 skips ? t.land : nullptr);
    if (t.any_varint && LaunchPbRunPrefix(t.term_chunk, (int)t.nchunks + 1, s) != 0) return -1;
    if (skips) {
        SPLIT_LAUNCH(pb_split_skip_kernel, dim3(t.nchunks), wg, t.exit, t.skip, t.skip_hops);
        SPLIT_LAUNCH(pb_split_chase_kernel, per_job, wave, t.skip, t.land);
        SPLIT_LAUNCH(pb_split_fill_kernel, dim3((t.nchunks + 63) / 64), wave, t.exit, t.land, t.entry, t.skip_hops,
                     t.nchunks);
    } else {
        SPLIT_LAUNCH(pb_split_chase_kernel, per_job, wave, t.exit, t.entry);
    }
    SPLIT_LAUNCH(pb_split_mark_kernel, dim3(t.nchunks), wg, t.entry, t.row_mask, t.row_chunk, t.bad, t.others);
    return LaunchPbRunPrefix(t.row_chunk, (int)t.nchunks + 1, s);
}

int LaunchPbRowsSplit(const PbSplitTables& t, hipStream_t s) {
    if (t.njobs <= 0) return 0;
    if (!t.res || split_front(t, s) != 0) return -1;
    const dim3 per_job((unsigned)(t.njobs + 63) / 64), wave(64), wg(kRunThreads);
    SPLIT_LAUNCH(pb_split_table_kernel, dim3(t.nchunks), wg, t.row_mask, t.row_chunk, t.exit, t.bad);
    if (t.any_varint) {
        SPLIT_LAUNCH(pb_split_varint_kernel<false>, dim3(t.nchunks), wg, t.exit, t.term_mask, t.term_group,
                     t.term_chunk, t.row_chunk, t.row_bias, t.bad, t.ok);
    }
    SPLIT_LAUNCH(pb_split_rows_kernel<false>, dim3(t.nrblocks), dim3(kPbSplitBlockRows), t.exit, t.term_mask,
                 t.term_group, t.term_chunk, t.row_chunk, t.block_sum, t.row_bias, t.ok);
    if (LaunchPbRunPrefix(t.block_sum, (int)t.nrblocks + 1, s) != 0) return -1;
    SPLIT_LAUNCH(pb_split_publish_kernel, per_job, wave, t.row_chunk, t.block_sum, t.bad, t.others, t.ok, t.res);
    SPLIT_LAUNCH(pb_split_rows_kernel<true>, dim3(t.nrblocks), dim3(kPbSplitBlockRows), t.exit, t.term_mask,
                 t.term_group, t.term_chunk, t.row_chunk, t.block_sum, t.row_bias, t.ok);
    if (t.any_varint) {
        SPLIT_LAUNCH(pb_split_varint_kernel<true>, dim3(t.nchunks), wg, t.exit, t.term_mask, t.term_group,
                     t.term_chunk, t.row_chunk, t.row_bias, t.bad, t.ok);
    }
    if (t.nochunks > 0) {
        SPLIT_LAUNCH(pb_split_place_kernel, dim3(t.nochunks), wg, t.exit, t.row_chunk, t.block_sum, t.ok);
    }
    return 0;
}

int LaunchPbRecordsSplit(const PbRecSplitTables& r, hipStream_t s) {
    const PbSplitTables& t = r.front;
    if (t.njobs <= 0) return 0;
    if (!r.jobs || !r.cols || !r.jobs_dev || !r.cols_dev || !r.specs || !r.entry || !r.bias || !r.rec_tag ||
        !r.block_sum || !r.absent || !r.res || r.ncols <= 0 || r.nrblocks == 0 || r.nrblocks > 0x7FFFFFFEu ||
        r.nbsums == 0 || r.nbsums > 0x7FFFFFFEu || t.any_varint != r.any_varint || split_front(t, s) != 0) {
        return -1;
    }
    const int most = t.njobs > r.ncols ? t.njobs : r.ncols;
    const dim3 per_job((unsigned)(t.njobs + 63) / 64), wave(64), wg(kRunThreads), rblocks(r.nrblocks);
    hipLaunchKernelGGL(pb_recsplit_init_kernel, dim3((unsigned)(most + 63) / 64), wave, 0, s, r.jobs, t.njobs,
                       r.jobs_dev, r.cols, r.ncols, r.cols_dev, r.specs, r.absent, r.block_sum, r.nbsums);
    if (hipGetLastError() != hipSuccess) return -1;
    SPLIT_LAUNCH(pb_recsplit_table_kernel, dim3(t.nchunks), wg, r.jobs_dev, r.specs, t.row_mask, t.row_chunk, r.entry,
                 r.rec_tag, t.bad);
    if (r.any_varint) {
        SPLIT_LAUNCH(pb_recsplit_varint_kernel<false>, dim3(t.nchunks), wg, r.jobs_dev, r.cols_dev, r.entry, r.rec_tag,
                     r.bias, t.term_mask, t.term_group, t.term_chunk, t.row_chunk, t.bad, t.ok);
    }
    SPLIT_LAUNCH(pb_recsplit_rows_kernel<false>, rblocks, dim3(kPbSplitBlockRows), r.jobs_dev, r.cols_dev, r.entry,
                 t.term_mask, t.term_group, t.term_chunk, t.row_chunk, r.block_sum, r.bias, r.absent, t.ok);
    if (LaunchPbRunPrefix(r.block_sum, (int)r.nbsums + 1, s) != 0) return -1;
    SPLIT_LAUNCH(pb_recsplit_publish_kernel, per_job, wave, r.jobs_dev, r.cols_dev, t.row_chunk, r.block_sum, r.absent,
                 t.bad, t.others, t.ok, r.res);
    SPLIT_LAUNCH(pb_recsplit_rows_kernel<true>, rblocks, dim3(kPbSplitBlockRows), r.jobs_dev, r.cols_dev, r.entry,
                 t.term_mask, t.term_group, t.term_chunk, t.row_chunk, r.block_sum, r.bias, r.absent, t.ok);
    if (r.any_varint) {
        SPLIT_LAUNCH(pb_recsplit_varint_kernel<true>, dim3(t.nchunks), wg, r.jobs_dev, r.cols_dev, r.entry, r.rec_tag,
                     r.bias, t.term_mask, t.term_group, t.term_chunk, t.row_chunk, t.bad, t.ok);
    }
    if (r.nochunks > 0) {
        hipLaunchKernelGGL(pb_recsplit_place_kernel, dim3(r.nochunks), wg, 0, s, t.jobs_dev, r.jobs_dev, r.cols_dev,
                           r.ncols, r.entry, t.row_chunk, r.block_sum, t.ok);
        if (hipGetLastError() != hipSuccess) return -1;
    }
    return 0;
}
#undef SPLIT_LAUNCH

int LaunchPbRecordsBuild(const PbRecordsTables& t, hipStream_t s) {
    if (t.njobs <= 0) return 0;
    if (!t.jobs || !t.cols || t.ncols <= 0 || !t.jobs_dev || !t.cols_dev || !t.row_size || !t.col_pay ||
        !t.col_delta || !t.block_off || !t.bad || !t.res || t.nrblocks == 0 || (t.ngroups > 0 && !t.groups) ||
        t.ngroups > 0x7FFFFFFFu) {
        return -1;
    }
    const int most = t.njobs > t.ncols ? t.njobs : t.ncols;
    hipLaunchKernelGGL(pb_records_init_kernel, dim3((unsigned)(most + 63) / 64), dim3(64), 0, s, t.jobs, t.njobs, t.cols,
                       t.ncols, t.jobs_dev, t.cols_dev, t.groups, t.bad);
    if (hipGetLastError() != hipSuccess) return -1;
    if (t.ngroups > 0) {
        if (t.nchunks > 0) {
            hipLaunchKernelGGL(pb_rows_size_kernel, dim3(t.nchunks), dim3(kRunThreads), 0, s, t.cols_dev, t.ncols,
                               t.groups);
            if (hipGetLastError() != hipSuccess) return -1;
        }
        if (LaunchPbRunPrefix(t.groups, (int)t.ngroups, s) != 0) return -1;
    }
    hipLaunchKernelGGL(pb_records_measure_kernel, dim3(t.nrblocks), dim3(kPbRowsBlockRows), 0, s, t.jobs_dev, t.njobs,
                       t.cols_dev, t.groups, t.row_size, t.col_pay, t.col_delta, t.block_off, t.bad);
    if (hipGetLastError() != hipSuccess) return -1;
    if (LaunchPbRunPrefix(t.block_off, (int)(t.nrblocks + (uint32_t)t.njobs), s) != 0) return -1;
    hipLaunchKernelGGL(pb_records_heads_kernel, dim3(t.nrblocks), dim3(kPbRowsBlockRows), 0, s, t.jobs_dev, t.njobs,
                       t.cols_dev, t.row_size, t.col_pay, t.col_delta, t.block_off, t.bad, t.res);
    if (hipGetLastError() != hipSuccess) return -1;
    if (t.nchunks == 0) return 0;
    hipLaunchKernelGGL(pb_records_place_kernel, dim3(t.nchunks), dim3(kRunThreads), 0, s, t.jobs_dev, t.cols_dev,
                       t.ncols, t.groups, t.block_off, t.col_delta, t.bad, t.res);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int LaunchPbMsgEncode(const PbMsgTables& t, hipStream_t s) {
    if (t.nmsgs <= 0) return 0;
    if (!t.prefix || !t.base || t.nfields < 0 || t.nchunks < 0) return -1;
    const int size_wgs = (t.nchunks + kRunThreads / 64 - 1) / (kRunThreads / 64);
    const int size_grid = size_wgs < 1 ? 1 : (size_wgs < 2048 ? size_wgs : 2048);
    hipLaunchKernelGGL(pb_msg_size_kernel, dim3((unsigned)size_grid), dim3(kRunThreads), 0, s, t.chunks, t.nchunks,
                       t.prefix);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(pb_run_prefix_kernel, dim3(1), dim3(kPrefixThreads), 0, s, t.prefix, t.nchunks + 1);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(pb_msg_layout_kernel, dim3((unsigned)t.nmsgs), dim3(64), 0, s, t.msgs, t.fields, t.prefix,
                       t.base, t.res, t.fres);
    if (hipGetLastError() != hipSuccess) return -1;
    if (t.nchunks == 0) return 0;
    hipLaunchKernelGGL(pb_msg_place_kernel, dim3((unsigned)t.nchunks), dim3(kRunThreads), 0, s, t.chunks, t.fields,
                       t.prefix, t.base, t.res);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int LaunchPbRunPrefix(uint32_t* prefix, int n, hipStream_t s) {
    if (n <= 0) return 0;
    if (!prefix) return -1;
    hipLaunchKernelGGL(pb_run_prefix_kernel, dim3(1), dim3(kPrefixThreads), 0, s, prefix, n);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int LaunchPbRunDecode(const PbRunDecodeChunk* chunks, int n, uint32_t* counts, uint32_t* prefix, int32_t* err,
                      hipStream_t s) {
    if (n <= 0) return 0;
    if (!prefix) return -1;
    // a wave per chunk, 8 workgroups (32 waves) per CU at most; the waves
    // stride over the rest
    const int count_wgs = (n + kRunThreads / 64 - 1) / (kRunThreads / 64);
    const int count_grid = count_wgs < 2048 ? count_wgs : 2048;
    const int decode_grid = n < 1024 ? n : 1024;  // 4 resident per CU (37 KiB of LDS each)
    hipLaunchKernelGGL(pb_run_count_kernel, dim3((unsigned)count_grid), dim3(kRunThreads), 0, s, chunks, n, counts,
                       prefix);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(pb_run_prefix_kernel, dim3(1), dim3(kPrefixThreads), 0, s, prefix, n);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(pb_run_decode_kernel, dim3((unsigned)decode_grid), dim3(kRunThreads), 0, s, chunks, n, prefix,
                       err);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int LaunchPbRunEncode(const PbRunChunk* chunks, int n, int32_t* err, hipStream_t s) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(pb_run_encode_kernel, dim3((unsigned)n), dim3(kRunThreads), 0, s, chunks, err);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int LaunchPbScan(const uint8_t* buf, uint64_t buf_len, const int64_t* offsets_dev, int64_t n, uint32_t max_fields,
                 uint64_t* fields, int32_t* nfields, hipStream_t s) {
    if (n <= 0) return 0;
    if (max_fields == 0) return -1;
    const int64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(pb_scan_kernel, dim3((unsigned)blocks), dim3(256), 0, s, buf, buf_len, offsets_dev, n,
                       max_fields, fields, nfields);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int LaunchPbScanPtrs(const PbScanJob* jobs, int64_t n, uint32_t max_fields, uint64_t* fields, int32_t* nfields,
                     hipStream_t s) {
    if (n <= 0) return 0;
    if (max_fields == 0) return -1;
    const int64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(pb_scan_ptrs_kernel, dim3((unsigned)blocks), dim3(256), 0, s, jobs, n, max_fields, fields,
                       nfields);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace gpu
}  // namespace mrpc
