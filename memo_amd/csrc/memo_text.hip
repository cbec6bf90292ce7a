// memo_text.hip -- `memo view` reading: the text of a conservation result (one integer per line), parsed on the device it will be
// binned on.  Counterpart of src/plot_conservation.py:40-49 (fileReader + list(map(int, ...))) for the grammar `memo query` writes;
// everything else is reported (first_odd_offset) and read by the caller as the reference reads it (memo_amd/view.py).
//
// The whole text is resident, so no kernel knows about the pieces it arrived in.  Three passes:
//   text_count_kernel   per 16 KB tile: its line terminators counted, every byte validated         (reads the text once)
//   the scan            memo::scan_tile_counts (memo_compact.hip): exclusive scan of the tile counts, one workgroup
//   text_parse_kernel   the tile + a 48-byte left halo staged in LDS; each line is parsed by the lane that owns its terminator,
//                       reading backwards; line number = tile base + rank of the terminator in the workgroup  (reads it again)
// The count's tail and the ranks are memo_compact.h's device pieces (store_tile_count, rank_flags).
// A last line without \n is ended by the end of the text: position nbytes is staged as a \n then, and as it may open a tile of
// its own the grid is nbytes / 16384 + 1 tiles.  Bytes behind it are staged as 0xFF, which is neither a terminator nor validated.
// Halo: 32 bytes of line, its \r, the terminator before it -- 34 bytes, rounded up to the 16-byte load.
#include "memo_compact.h"

using namespace memo;

namespace {

constexpr int kTile = 16384, kHalo = 48, kWaveSpan = kTile / 4, kIterSpan = 1024;  // 256 lanes x 16 B x 4; a wave owns 4 KB in a row
static_assert(kCompactIters == 4 && kCompactThreads == 256, "the tile is cut as memo_compact.h's device pieces cut theirs");
constexpr int kMaxLine = 32, kMaxDigits = 9;
constexpr unsigned long long kNoOdd = ~0ull;

__device__ __forceinline__ uint32_t byte_of(const uint4 &v, int j) {
    const uint32_t w = j < 4 ? v.x : j < 8 ? v.y : j < 12 ? v.z : v.w;
    return (w >> (8 * (j & 3))) & 0xFFu;
}

// the 16 staged bytes at pos (a multiple of 16, >= 0): the text, a \n at nbytes when the last line has none, 0xFF behind
__device__ __forceinline__ uint4 load_chunk(const char *__restrict__ text, int64_t pos, int64_t nbytes, bool open_end) {
    if (pos + 16 <= nbytes) return *reinterpret_cast<const uint4 *>(text + pos);
    uint32_t w[4] = {~0u, ~0u, ~0u, ~0u};
    if (pos <= nbytes) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int64_t p = pos + j;
            const uint32_t b = p < nbytes ? (uint32_t)(unsigned char)text[p] : (p == nbytes && open_end ? (uint32_t)'\n' : 0xFFu);
            w[j >> 2] = (w[j >> 2] & ~(0xFFu << (8 * (j & 3)))) | (b << (8 * (j & 3)));
        }
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ bool open_ended(const char *__restrict__ text, int64_t nbytes) { return nbytes > 0 && text[nbytes - 1] != '\n'; }

__device__ __forceinline__ int64_t chunk_pos(int64_t tile0, int it) {
    return tile0 + (threadIdx.x >> 6) * kWaveSpan + it * kIterSpan + (threadIdx.x & 63) * 16;
}

// one atomic per wave, and none at all on a text without oddities
__device__ __forceinline__ void report_odd(unsigned long long odd, unsigned long long *first_odd) {
    if (!__any(odd != kNoOdd)) return;
    for (int off = 32; off; off >>= 1) {
        const unsigned long long t = (unsigned long long)__shfl_xor((long long)odd, off, 64);
        odd = t < odd ? t : odd;
    }
    if ((threadIdx.x & 63) == 0) atomicMin(first_odd, odd);
}

__global__ __launch_bounds__(256) void text_count_kernel(const char *__restrict__ text, int64_t nbytes, uint32_t *__restrict__ counts,
                                                         unsigned long long *first_odd) {
    const int64_t tile0 = (int64_t)blockIdx.x * kTile;
    const bool open_end = open_ended(text, nbytes);
    uint4 v[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) v[it] = load_chunk(text, chunk_pos(tile0, it), nbytes, open_end);
    uint32_t n = 0;
    unsigned long long odd = kNoOdd;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int64_t pos = chunk_pos(tile0, it);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint32_t b = byte_of(v[it], j);
            const int64_t p = pos + j;
            n += b == '\n';
            bool ok = b - '0' < 10u || b == ' ' || b == '\t' || b == '\n';
            if (b == '\r' && p + 1 < nbytes)  // (the staged \n at nbytes follows no \r: the file has none there)
                ok = (j < 15 ? byte_of(v[it], j + 1) : (uint32_t)(unsigned char)text[p + 1]) == '\n';
            if (!ok && p < nbytes && (unsigned long long)p < odd) odd = (unsigned long long)p;
        }
    }
    report_odd(odd, first_odd);
    store_tile_count(n, counts);
}

__global__ __launch_bounds__(256) void text_parse_kernel(const char *__restrict__ text, int64_t nbytes, const int64_t *__restrict__ bases,
                                                         uint16_t *__restrict__ vec, int64_t cap, unsigned long long *first_odd) {
    // one array (the tile behind its halo, then the four waves' terminator counts)
    __shared__ uint4 staged[(kHalo + kTile) / 16 + 1];
    unsigned char *const sm = reinterpret_cast<unsigned char *>(staged);
    uint32_t *const wtot = reinterpret_cast<uint32_t *>(staged + (kHalo + kTile) / 16);
    const int64_t tile0 = (int64_t)blockIdx.x * kTile;
    const bool open_end = open_ended(text, nbytes);
    if (threadIdx.x < kHalo / 16)  // (tile0 <= nbytes: the halo lies inside the text; before the text: its beginning starts a line)
        staged[threadIdx.x] = tile0 ? *reinterpret_cast<const uint4 *>(text + tile0 - kHalo + 16 * threadIdx.x)
                                    : make_uint4(0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au);
    uint4 v[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) v[it] = load_chunk(text, chunk_pos(tile0, it), nbytes, open_end);
#pragma unroll
    for (int it = 0; it < 4; ++it) staged[(kHalo + chunk_pos(0, it)) / 16] = v[it];
    // the terminators of a lane's loads, and their ranks among the tile's
    uint32_t mask[4], rank[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        uint32_t m = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) m |= (byte_of(v[it], j) == '\n' ? 1u : 0u) << j;
        mask[it] = m;
    }
    const int64_t line = bases[blockIdx.x] + rank_flags<16>(mask, rank, wtot);
    unsigned long long odd = kNoOdd;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        int64_t idx = line + rank[it];
        const int at = kHalo + (int)chunk_pos(0, it);
        for (uint32_t m = mask[it]; m; m &= m - 1, ++idx) {
            const int t = at + __builtin_ctz(m);  // the terminator; at most 1 + 33 + 10 bytes before it are read: never below sm[3]
            int q = t - 1, len = 0, digits = 0;
            uint32_t b = sm[q], val = 0, mul = 1;
            if (b == '\r') b = sm[--q];
            for (; (b == ' ' || b == '\t') && len <= kMaxLine; ++len) b = sm[--q];
            for (; b - '0' < 10u && digits <= kMaxDigits; ++digits, ++len, mul *= 10) {
                val += (b - '0') * mul;
                b = sm[--q];
            }
            for (; (b == ' ' || b == '\t') && len <= kMaxLine; ++len) b = sm[--q];
            if (b != '\n' || digits == 0 || digits > kMaxDigits || len > kMaxLine) {
                const unsigned long long p = (unsigned long long)(tile0 + t - kHalo);
                odd = p < odd ? p : odd;
            }
            if (idx < cap) vec[idx] = (uint16_t)(val < 65535u ? val : 65535u);
        }
    }
    report_odd(odd, first_odd);
}

}  // namespace

extern "C" {

int memo_parse_conservation_text_dev(const char *d_text, int64_t nbytes, uint16_t *d_vec, int64_t cap, int64_t *lines,
                                     int64_t *first_odd_offset, int32_t device, void *stream) {
    if (!lines || !first_odd_offset) return fail(MEMO_EINVAL, "lines / first_odd_offset is NULL");
    *lines = 0;
    *first_odd_offset = -1;
    if (nbytes < 0 || cap < 0 || (nbytes && !d_text) || (cap && !d_vec)) return fail(MEMO_EINVAL, "bad text arguments");
    if (reinterpret_cast<uintptr_t>(d_text) & 15) return fail(MEMO_EINVAL, "d_text must be 16-byte aligned");
    if (!nbytes) return MEMO_OK;
    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t ntiles = nbytes / kTile + 1;
    if (ntiles > INT32_MAX) return fail(MEMO_EINVAL, "a text of %lld bytes is too long", (long long)nbytes);
    // one allocation: [lines, first odd offset], the tiles' bases, their counts
    DevPtr<int64_t> work;
    HIP_TRY(work.alloc((size_t)(2 + ntiles + (ntiles + 1) / 2)));
    int64_t *d_res = work, *d_bases = d_res + 2;
    uint32_t *d_counts = reinterpret_cast<uint32_t *>(d_bases + ntiles);
    unsigned long long *d_odd = reinterpret_cast<unsigned long long *>(d_res + 1);
    HIP_TRY(hipMemsetAsync(d_res, 0xFF, 16, st));
    hipLaunchKernelGGL(text_count_kernel, dim3((unsigned)ntiles), dim3(256), 0, st, d_text, nbytes, d_counts, d_odd);
    HIP_TRY(hipGetLastError());
    HIP_TRY(scan_tile_counts(d_counts, ntiles, d_bases, d_res, st));
    HIP_TRY(hipMemcpyAsync(lines, d_res, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (cap < *lines) return fail(MEMO_EINVAL, "the text has %lld lines: d_vec holds %lld", (long long)*lines, (long long)cap);
    hipLaunchKernelGGL(text_parse_kernel, dim3((unsigned)ntiles), dim3(256), 0, st, d_text, nbytes, d_bases, d_vec, cap, d_odd);
    HIP_TRY(hipGetLastError());
    unsigned long long odd = kNoOdd;
    HIP_TRY(hipMemcpyAsync(&odd, d_odd, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *first_odd_offset = odd == kNoOdd ? -1 : (int64_t)odd;
    return MEMO_OK;
}

}  // extern "C"
