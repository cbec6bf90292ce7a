// memo_tracks.hip -- `memo tracks`: per-genome k-mer presence along the pivot, binned, of a membership result that is still in HBM,
//     counts[g][b] += #{ p in [first, first + L) : edges[b] <= p < edges[b + 1] and bit g of row p - first is set }      uint64 [num_docs][bins]
// so that num_docs x bins integers and not L rows leave the device.  No counterpart in the reference: the membership counterpart of
// the binning kernel of `memo view` (memo_text.hip), and the third reduction over positions on the planes of memo_planes.h.
//
// The launcher turns the edges into slice coordinates (edge - first, clamped to [0, L]) before it uploads them: the bins then cut
// [0, L) into consecutive runs, every position in exactly one bin, and the kernel knows neither `first` nor the window.
//
// One tile = PW position words = 32 PW positions, PW as memo_collect.hip chooses it (16 up to 16 genome words, 8 up to 32, 4 up to
// 64: at most 256 blocks a tile, one a lane).  A workgroup of 256 lanes takes a run of consecutive tiles.  Lane i owns the genomes
// i, i + 256, ... (KG = 1, 2, 4 or 8 of them) and keeps one 32-bit count for each: the count of the bin the workgroup is in.
//   - Once per workgroup: a binary search over the edges for the bin of its first position (every lane the same search).
//   - Per tile: stage the planes (stage_plane_block: one load per row word, rows at or past L as zeros, bits at or above num_docs
//     masked), then walk the tile bin by bin.  A piece [p, e) of the tile inside one bin is counted by each lane for its genomes:
//     one LDS read, one and with the piece's mask and one popcount per position word of the piece.  When the bin ends, the lane adds
//     its counts to counts[g][bin] with one 64-bit atomic each (none for a count of zero) and moves to the next edge.
//   - A bin that goes on behind the tile keeps its counts in the registers; they leave when it ends, or with the workgroup.
// So a workgroup issues at most num_docs x (bins it touches) atomics, whatever its positions are: with bins wider than its run
// one or two per genome.  Narrow bins take the same walk, piece by piece: a bin of one position costs each lane one read, one
// popcount and at most one atomic per genome, empty bins one edge load each (DESIGN.md 10.12 has both times).
//
// Conditions the code holds:
//   - no workgroup waits for another: no look-back, no flag in memory, no cooperative launch
//   - nothing is read outside d_bits[0 .. L * W) and edges[0 .. bins]: the walk stops in the bin that holds the last position, and
//     the last edge is L
//   - a d_bits that is not 16-byte aligned is MEMO_EINVAL before any launch; so are decreasing edges and a slice that leaves them
//   - L == 0 launches nothing and leaves d_counts as it was
//   - L and positions are int64; the table is 64-bit; integer adds are exact in any order, so the table depends neither on the
//     slices nor on the launch shape
//   - the 32-bit counts cannot wrap: one gains at most 1 per position, and the launcher refuses (MEMO_EINVAL) what would give a
//     workgroup more than 2^31 positions
//   - scratch: the uploaded edges, (bins + 1) x 8 bytes, at most 8 MiB + 8; DevPtr owns them; an allocation that fails is MEMO_EHIP
//     with the bytes asked for, and nothing stays allocated
//   - vector stores and plain C++ only
#include <algorithm>
#include <vector>

#include "memo_planes.h"

using namespace memo;

namespace memo {
thread_local int g_tracks_timed = 0;    // 1 = an event pair around the launch (memo_debug_tracks_times)
thread_local float g_tracks_ms = 0.f;   // ... of the last such call
}

namespace {

constexpr int kThreads = 256;
constexpr int kMaxDocs = 2048;   // 64 genome words: the planes of a 4-word tile are 36 KiB; eight genomes a lane
constexpr int kMaxBins = 1 << 20;
constexpr int kMaxGridX = 1024;  // workgroups at most
constexpr int64_t kMaxPositionsPerWg = (int64_t)1 << 31;

struct TracksArgs {
    const uint32_t *bits;
    int64_t L, ntiles, tiles_per_wg;
    int W, N, bins;
    int pitch;             // LDS words per position word
    const int64_t *edges;  // [bins + 1], slice coordinates, non-decreasing, edges[0] == 0 and edges[bins] == L
    uint64_t *counts;      // [N][bins]
};

inline int position_words(int W) { return W <= 16 ? 16 : W <= 32 ? 8 : 4; }

template <int PW, int KG>
__global__ __launch_bounds__(kThreads) void tracks_kernel(const TracksArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint32_t planes[];
    constexpr int kTile = 32 * PW;
    const int64_t t0 = (int64_t)blockIdx.x * A.tiles_per_wg, t1 = min(t0 + A.tiles_per_wg, A.ntiles);
    // the bin of the workgroup's first position: the first b with edges[b + 1] > t0 * kTile (there is one: edges[bins] == L)
    int b = 0;
    {
        const int64_t p = t0 * kTile;
        int hi = A.bins - 1;
        while (b < hi) {
            const int mid = (b + hi) >> 1;
            if (A.edges[mid + 1] > p) hi = mid;
            else b = mid + 1;
        }
    }
    int64_t bin_end = A.edges[b + 1];
    int at[KG];  // where the lane's genomes lie in a position word's row
#pragma unroll
    for (int j = 0; j < KG; ++j) {
        const int g = min((int)threadIdx.x + kThreads * j, A.N - 1);
        at[j] = kPlaneBlockPitch * (g >> 5) + (g & 31);
    }
    uint32_t acc[KG] = {};
    auto flush = [&](int bin) {
#pragma unroll
        for (int j = 0; j < KG; ++j) {
            const int g = (int)threadIdx.x + kThreads * j;
            if (g < A.N && acc[j]) atomicAdd(reinterpret_cast<unsigned long long *>(A.counts) + (int64_t)g * A.bins + bin, (unsigned long long)acc[j]);
            acc[j] = 0;
        }
    };
    const int staged = A.W * PW;  // blocks a tile has: at most one a lane
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t ts = t * kTile, te = min(ts + kTile, A.L);
        // (few genome words are one wave's work or less: the wave that does it changes with the tile, as in cooc_kernel)
        for (int blk = (threadIdx.x + 64 * (int)(t & 3)) & (kThreads - 1); blk < staged; blk += kThreads) {
            const int w = blk % A.W, P = blk / A.W;
            stage_plane_block(A.bits, A.L, A.W, A.N, w, ts + 32 * P, planes + P * A.pitch + kPlaneBlockPitch * w);
        }
        __syncthreads();
        int64_t p = ts;
        for (;;) {
            const int64_t e = min(bin_end, te);
            if (e > p) {  // the piece [p, e) of the tile lies in bin b
                const int lo = (int)(p - ts), hi = (int)(e - ts);  // 0 <= lo < hi <= kTile
                for (int P = lo >> 5; P <= (hi - 1) >> 5; ++P) {
                    const int from = max(lo - 32 * P, 0), to = min(hi - 32 * P, 32);  // 0 <= from < to <= 32
                    const uint32_t mask = (0xFFFFFFFFu >> (32 - (to - from))) << from;
                    const uint32_t *row = planes + P * A.pitch;
#pragma unroll
                    for (int j = 0; j < KG; ++j) acc[j] += (uint32_t)__popc(row[at[j]] & mask);
                }
                p = e;
            }
            if (p >= te) break;  // the tile is done; bin b may go on in the next one
            flush(b);            // bin_end <= p < L: the bin is done, and it is not the last
            bin_end = A.edges[++b + 1];
        }
        __syncthreads();
    }
    flush(b);
}

template <int PW, int KG>
void launch(const TracksArgs &A, int gx, hipStream_t st) {
    hipLaunchKernelGGL((tracks_kernel<PW, KG>), dim3((unsigned)gx), dim3(kThreads), (size_t)PW * A.pitch * sizeof(uint32_t), st, A);
}

template <int PW>
void launch_pw(const TracksArgs &A, int gx, hipStream_t st) {
    const int kg = (A.N + kThreads - 1) / kThreads;
    if (kg <= 1) launch<PW, 1>(A, gx, st);
    else if (kg <= 2) launch<PW, 2>(A, gx, st);
    else if (kg <= 4) launch<PW, 4>(A, gx, st);
    else launch<PW, 8>(A, gx, st);
}

}  // namespace

extern "C" {

int32_t memo_tracks_tile(int32_t words) { return 32 * position_words(words); }

int memo_tracks_dev(const uint32_t *d_bits, int64_t L, int32_t num_docs, int64_t first, const int64_t *edges_host, int32_t bins,
                    uint64_t *d_counts, int32_t device, void *stream) {
    if (num_docs < 1 || num_docs > kMaxDocs) return fail(MEMO_EINVAL, "num_docs must be in [1, %d] (num_docs = %d)", kMaxDocs, num_docs);
    if (bins < 1 || bins > kMaxBins) return fail(MEMO_EINVAL, "bins must be in [1, %d] (bins = %d)", kMaxBins, bins);
    if (L < 0 || (L && !d_bits)) return fail(MEMO_EINVAL, "bad membership result (L = %lld)", (long long)L);
    if (!edges_host) return fail(MEMO_EINVAL, "edges is NULL");
    if (!d_counts || (reinterpret_cast<uintptr_t>(d_counts) & 7)) return fail(MEMO_EINVAL, "d_counts is NULL or not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_bits) & 15) return fail(MEMO_EINVAL, "d_bits must be 16-byte aligned");
    for (int32_t b = 0; b < bins; ++b)
        if (edges_host[b + 1] < edges_host[b])
            return fail(MEMO_EINVAL, "the bin edges decrease: edge %d is %lld, edge %d is %lld", b, (long long)edges_host[b], b + 1,
                        (long long)edges_host[b + 1]);
    // (first + L cannot wrap where it matters: L <= edges[bins] - first is asked instead)
    if (first < edges_host[0] || first > edges_host[bins] || L > edges_host[bins] - first)
        return fail(MEMO_EINVAL, "the slice [%lld, %lld + %lld) leaves the bin edges [%lld, %lld)", (long long)first, (long long)first,
                    (long long)L, (long long)edges_host[0], (long long)edges_host[bins]);
    if (!L) return MEMO_OK;

    TracksArgs A = {};
    A.bits = d_bits;
    A.L = L;
    A.W = (num_docs + 31) / 32;
    A.N = num_docs;
    A.bins = bins;
    A.pitch = kPlaneBlockPitch * A.W + 4;
    A.counts = d_counts;
    const int pw = position_words(A.W), tile = 32 * pw;
    A.ntiles = (L + tile - 1) / tile;
    const int64_t cap = std::min<int64_t>(kMaxGridX, A.ntiles);
    A.tiles_per_wg = (A.ntiles + cap - 1) / cap;
    if (A.tiles_per_wg * tile > kMaxPositionsPerWg) return fail(MEMO_EINVAL, "a result of %lld positions is too long", (long long)L);
    const int gx = (int)((A.ntiles + A.tiles_per_wg - 1) / A.tiles_per_wg);
    // the edges in slice coordinates: [0, L] cut into consecutive bins, the first edge 0 and the last one L
    std::vector<int64_t> rel((size_t)bins + 1);
    for (int32_t b = 0; b <= bins; ++b) rel[b] = std::min<int64_t>(std::max<int64_t>(edges_host[b] - first, 0), L);

    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DevPtr<int64_t> d_edges;
    if (hipError_t err = d_edges.alloc(rel.size()); err != hipSuccess)
        return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the edges of %d bins: %s", rel.size() * sizeof(int64_t), bins, hipGetErrorString(err));
    HIP_TRY(hipMemcpyAsync(d_edges, rel.data(), rel.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    A.edges = d_edges;
    Laps laps(st, g_tracks_timed, &g_tracks_ms);
    if (int rc = laps.start()) return rc;
    if (pw == 16) launch_pw<16>(A, gx, st);
    else if (pw == 8) launch_pw<8>(A, gx, st);
    else launch_pw<4>(A, gx, st);
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(0)) return rc;
    HIP_TRY(hipStreamSynchronize(st));  // (rel and d_edges go with this frame)
    return MEMO_OK;
}

}  // extern "C"
