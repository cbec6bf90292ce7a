// memo_cover.hip -- `memo cover`: `memo panel` at every k of [kmin, kmax] at once -- the greedy cover of a window's match lengths, one
// step at a time, on weight planes that stay in HBM.  With span = kmax - kmin + 1 and
//     w[g][p] = max(0, min(len[g][p], kmax) - (kmin - 1))        the number of k in [kmin, kmax] at which genome g holds the k-mer at p
// the two masks of memo_panel.hip, stacked over every k, are two integer vectors over the positions: core (the smallest weight taken so
// far, span at first) and covered (the largest, 0 at first).  No counterpart in the reference.  The bit planes of memo_panel.hip cannot
// carry this: a cell is an integer of 2 bytes (span <= 65535) or 4, sixteen or thirty-two times the bytes of a bit, and a step is a
// stream of min, max, saturating subtract and add over them.  One kernel template over the cell type serves both widths.
//
// Plane i is `pitch` cells at d_weights + i * pitch * cell_bytes; pitch is a multiple of a QUAD, 16 / cell_bytes cells (8 or 4).  Only
// the genomes a caller names get a plane: the planes are numbered as the caller's list, not as the index's genomes.
//
//   memo_cover_weights_dev  one finished slice of `memo lengths`, uint32 [num_docs][pitch_src] -> cells [cell0, cell0 + Ls) of the
//       resident planes [0, n_list): plane i receives w[list[i]], narrowed to the cell type (a length above kmax counts as kmax: a
//       finished plane is not trusted to be capped).  cell0 is a multiple of 8, so that a quad of the slice is a quad of the plane: a
//       lane takes one quad -- 16 or 32 bytes of lengths in 16-byte loads, one 16-byte store -- and the ragged end goes cell by cell.
//       grid.x walks the quads, grid.y the list.  Nothing outside [cell0, cell0 + Ls) of any plane is written.
//   memo_cover_begin_dev    what no slice writes: the pad cells [L, the next multiple of a quad) of every plane as zeros, core as span
//       below L and zeros in the pad, covered as zeros.
//   memo_cover_score_dev    for a host list of plane numbers (repeats are legal)
//           new = sum over p of max(0, w[p] - covered[p])          kept = sum over p of min(w[p], core[p])
//       literally, for ANY cell values (max(0, w - c) is computed as max(w, c) - c, which cannot wrap).  memo_panel_score_dev's shape: a
//       workgroup takes a span of the quads (grid.x) and a block of kBlock = 8 candidates (grid.y); a lane reads 16 bytes of each mask
//       once per block and 16 bytes of each of the block's planes, all loads issued before the arithmetic (a block's tail repeats its
//       first candidate; those sums never leave).  Then a 64-bit wave reduce, the four waves through LDS, and 64-bit partials
//       [grid.x][n_list][2]; cover_reduce_kernel sums them over grid.x, one wave a cell.
//   memo_cover_take_dev     core = min(core, w), covered = max(covered, w) in place (a quad is read and written by one lane), and the
//       two new sums by the same partials and reduce launch.
//
// Exactness.  Every sum is exact for any cell values, any span up to 2^31 - 1 and any number of cells up to 2^31 - 1 (the sums of
// weights stay below 2^62; those of arbitrary 4-byte cells below 2^63).  How a lane accumulates:
//   2-byte cells   32-bit lane sums.  A quad adds at most 8 x 65535 < 2^19 to one, and a lane takes at most kMaxPasses16 = 8192 quads
//                  (a workgroup at most 2^21 quads, 2^24 cells), so a lane sum stays below 2^32.  The launcher raises grid.x until that
//                  holds -- at 2^31 cells it needs 128 workgroups along the cells, which take comes to anyway and score is given even
//                  where the scratch cap asked for fewer.  The lane sums are widened to 64 bits before the wave reduce.
//   4-byte cells   64-bit lane sums: a quad's four terms are added in 64 bits.  No bound is needed.
// The wave reduce, the workgroup's sum, the partials and the reduce launch are 64-bit for both.
//
// Conditions the code holds:
//   - no workgroup waits for another: no look-back, no flag in memory, no cooperative launch
//   - no global atomics: every partial and every output cell has one owner, and the stream orders the launches
//   - vector loads and stores and plain C++ only
//   - 64-bit plane indexing: plane number x pitch and every cell offset are int64
//   - weights_dev reads cells [0, Ls) of the planes list[i] of the lengths and nothing else of them; score and take read cells
//     [0, cells) of a plane and of the masks, cells a multiple of a quad and at most pitch
//   - MEMO_EINVAL before any launch leaves planes, masks and outputs as they were: a base that is NULL or not 16-byte aligned, a pitch
//     that is no multiple of a quad, a cell range that leaves the pitch (a cell0 that is no multiple of 8), a cell_bytes other than 2
//     or 4, a span that does not fit the cell (or kmin, kmax outside 1 <= kmin <= kmax <= 2^31 - 1), a list entry out of range, n_list
//     outside [0, 65535], num_docs / num_planes outside [1, 2048]
//   - scratch: the partials (at most 64 MiB, grid.x gives way; up to 128 MiB where the bound of the 2-byte lane sums asks for more
//     workgroups than that), the uploaded list and the 64-bit results, one allocation that DevPtr owns; an allocation that fails is
//     MEMO_EHIP with the bytes asked for, and nothing stays allocated
#include <algorithm>

#include "memo_common.h"

using namespace memo;

namespace memo {
thread_local int g_cover_timed = 0;  // 1 = event pairs around the launches (memo_debug_cover_times), each launch waited for
thread_local float g_cover_ms[4] = {0.f, 0.f, 0.f, 0.f};  // ... of the last such call of each kind: weights, the score sweep, its reduce, take
}

namespace {

constexpr int kThreads = 256;
constexpr int kMaxDocs = 2048;
constexpr int kBlock = 8;                      // candidates a workgroup of the score kernel takes
constexpr int64_t kMaxPasses16 = 8192;         // quads of 2-byte cells a lane adds up in 32 bits: 8192 x 8 x 65535 < 2^32
constexpr int kTargetGroups = 2048;            // workgroups a score launch aims at: eight a CU
constexpr int kMaxGridX = 2048;
constexpr size_t kScratchCap = (size_t)64 << 20;
constexpr int kMaxList = 65535;
constexpr uint32_t kCapMax = 0x7FFFFFFFu;

template <typename Cell>
struct Quad;  // what 16 bytes of cells are to a lane
template <>
struct Quad<uint16_t> {
    static constexpr int kCells = 8;
    using Sum = uint32_t;  // a lane's (the bound: kMaxPasses16)
};
template <>
struct Quad<uint32_t> {
    static constexpr int kCells = 4;
    using Sum = uint64_t;
};

// cell i of a quad
template <typename Cell>
__device__ __forceinline__ uint32_t cell_of(const uint4 q, int i);
template <>
__device__ __forceinline__ uint32_t cell_of<uint16_t>(const uint4 q, int i) {
    const uint32_t w = i < 2 ? q.x : i < 4 ? q.y : i < 6 ? q.z : q.w;
    return (i & 1) ? w >> 16 : w & 0xFFFFu;
}
template <>
__device__ __forceinline__ uint32_t cell_of<uint32_t>(const uint4 q, int i) {
    return i == 0 ? q.x : i == 1 ? q.y : i == 2 ? q.z : q.w;
}

// the quad of the cellwise minima / maxima of two quads (of 2-byte cells: two cells a word, each half on its own)
template <typename Cell>
__device__ __forceinline__ uint32_t word_min(uint32_t a, uint32_t b) {
    if (sizeof(Cell) == 4) return min(a, b);
    return min(a & 0xFFFFu, b & 0xFFFFu) | (min(a >> 16, b >> 16) << 16);
}
template <typename Cell>
__device__ __forceinline__ uint32_t word_max(uint32_t a, uint32_t b) {
    if (sizeof(Cell) == 4) return max(a, b);
    return max(a & 0xFFFFu, b & 0xFFFFu) | (max(a >> 16, b >> 16) << 16);
}
template <typename Cell>
__device__ __forceinline__ uint4 quad_min(const uint4 a, const uint4 b) {
    return make_uint4(word_min<Cell>(a.x, b.x), word_min<Cell>(a.y, b.y), word_min<Cell>(a.z, b.z), word_min<Cell>(a.w, b.w));
}
template <typename Cell>
__device__ __forceinline__ uint4 quad_max(const uint4 a, const uint4 b) {
    return make_uint4(word_max<Cell>(a.x, b.x), word_max<Cell>(a.y, b.y), word_max<Cell>(a.z, b.z), word_max<Cell>(a.w, b.w));
}

// the sum of a quad's cells
template <typename Cell>
__device__ __forceinline__ typename Quad<Cell>::Sum quad_sum(const uint4 q) {
    typename Quad<Cell>::Sum s = 0;
#pragma unroll
    for (int i = 0; i < Quad<Cell>::kCells; ++i) s += cell_of<Cell>(q, i);
    return s;
}

// ------------------------------------------------------------------------------------------------------------------------------
// lengths -> weights
// ------------------------------------------------------------------------------------------------------------------------------
struct WeightsArgs {
    const uint32_t *lengths;
    int64_t Ls, pitch_src;
    uint32_t kmin, kmax;
    const uint16_t *list;  // [n_list], on the device
    void *weights;
    int64_t pitch, cell0;
};

__device__ __forceinline__ uint32_t weight_of(uint32_t len, uint32_t kmin, uint32_t kmax) {
    const uint32_t v = min(len, kmax);
    return v >= kmin ? v - (kmin - 1u) : 0u;
}

template <typename Cell>
__global__ __launch_bounds__(kThreads) void cover_weights_kernel(const WeightsArgs A) {
    constexpr int G = Quad<Cell>::kCells;
    const int64_t c = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * G;  // the quad's first cell of the slice
    if (c >= A.Ls) return;
    const uint32_t *src = A.lengths + (int64_t)A.list[blockIdx.y] * A.pitch_src + c;
    Cell *dst = static_cast<Cell *>(A.weights) + (int64_t)blockIdx.y * A.pitch + A.cell0 + c;
    if (c + G <= A.Ls) {
        uint32_t w[G];
#pragma unroll
        for (int j = 0; j < G; j += 4) {
            const uint4 v = *reinterpret_cast<const uint4 *>(src + j);
            w[j] = weight_of(v.x, A.kmin, A.kmax);
            w[j + 1] = weight_of(v.y, A.kmin, A.kmax);
            w[j + 2] = weight_of(v.z, A.kmin, A.kmax);
            w[j + 3] = weight_of(v.w, A.kmin, A.kmax);
        }
        if constexpr (G == 8)
            *reinterpret_cast<uint4 *>(dst) = make_uint4(w[0] | w[1] << 16, w[2] | w[3] << 16, w[4] | w[5] << 16, w[6] | w[7] << 16);
        else
            *reinterpret_cast<uint4 *>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        for (int j = 0; c + j < A.Ls; ++j) dst[j] = (Cell)weight_of(src[j], A.kmin, A.kmax);
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// the pads and the masks
// ------------------------------------------------------------------------------------------------------------------------------
template <typename Cell>
__global__ __launch_bounds__(kThreads) void cover_begin_kernel(Cell *weights, int64_t pitch, int n_planes, int64_t L, uint32_t span, Cell *core, Cell *covered) {
    constexpr int G = Quad<Cell>::kCells;
    const int64_t cells = (L + G - 1) / G * G;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < cells) {
        core[i] = i < L ? (Cell)span : (Cell)0;
        covered[i] = (Cell)0;
    }
    const int64_t pad = cells - L;  // 0 .. G - 1 cells a plane
    if (i < pad * n_planes) weights[(i / pad) * pitch + L + i % pad] = (Cell)0;
}

// ------------------------------------------------------------------------------------------------------------------------------
// score, take, and the reduce launch behind both
// ------------------------------------------------------------------------------------------------------------------------------
// the sum of v over the wave's 64 lanes, in every one of them (memo_panel.hip's wave_sum is 32-bit; these sums pass 2^32)
__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const uint32_t lo2 = (uint32_t)__shfl_xor((int)lo, m), hi2 = (uint32_t)__shfl_xor((int)hi, m);
        const uint64_t both = ((uint64_t)hi << 32 | lo) + ((uint64_t)hi2 << 32 | lo2);
        lo = (uint32_t)both;
        hi = (uint32_t)(both >> 32);
    }
    return (uint64_t)hi << 32 | lo;
}

// the workgroup's sums of VALUES values a lane: out[i] in lanes 0 .. VALUES - 1 of the workgroup's first wave (tid = i) on return
template <int VALUES, typename Sum>
__device__ __forceinline__ uint64_t group_sums(const Sum (&acc)[VALUES]) {
    __shared__ uint64_t wsum[kThreads / 64][VALUES];
#pragma unroll
    for (int i = 0; i < VALUES; ++i) {
        const uint64_t s = wave_sum((uint64_t)acc[i]);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6][i] = s;
    }
    __syncthreads();
    uint64_t total = 0;
    if (threadIdx.x < VALUES)
        for (int wv = 0; wv < kThreads / 64; ++wv) total += wsum[wv][threadIdx.x];
    return total;
}

struct ScoreArgs {
    const void *weights;
    int64_t pitch;                // cells
    int64_t quads, quads_per_wg;  // 16-byte quads of the masks, and of one workgroup's span (a multiple of kThreads)
    const void *core, *covered;
    const uint16_t *list;         // [n_list], on the device
    int n_list;
    uint64_t *partials;           // [grid.x][n_list][2]: new, kept
};

template <typename Cell>
__global__ __launch_bounds__(kThreads) void cover_score_kernel(const ScoreArgs A) {
    using Sum = typename Quad<Cell>::Sum;
    const int c0 = blockIdx.y * kBlock, nc = min(kBlock, A.n_list - c0);
    const uint4 *plane[kBlock];
#pragma unroll
    for (int c = 0; c < kBlock; ++c)
        plane[c] = reinterpret_cast<const uint4 *>(static_cast<const Cell *>(A.weights) + (int64_t)A.list[c0 + (c < nc ? c : 0)] * A.pitch);
    const uint4 *core = static_cast<const uint4 *>(A.core), *covered = static_cast<const uint4 *>(A.covered);
    Sum acc[2 * kBlock] = {};  // [2 c]: the sum of max(w, covered), from which the sum of covered goes at the end; [2 c + 1]: kept
    Sum seen_sum = 0;
    const int64_t q0 = (int64_t)blockIdx.x * A.quads_per_wg, q1 = min(q0 + A.quads_per_wg, A.quads);
    for (int64_t q = q0 + threadIdx.x; q < q1; q += kThreads) {
        const uint4 keep = core[q], seen = covered[q];
        uint4 p[kBlock];
#pragma unroll
        for (int c = 0; c < kBlock; ++c) p[c] = plane[c][q];
        seen_sum += quad_sum<Cell>(seen);
#pragma unroll
        for (int c = 0; c < kBlock; ++c) {
            acc[2 * c] += quad_sum<Cell>(quad_max<Cell>(p[c], seen));
            acc[2 * c + 1] += quad_sum<Cell>(quad_min<Cell>(p[c], keep));
        }
    }
#pragma unroll
    for (int c = 0; c < kBlock; ++c) acc[2 * c] -= seen_sum;  // max(w, c) - c = max(0, w - c), term by term: the difference cannot wrap
    const uint64_t total = group_sums(acc);
    if ((int)threadIdx.x < 2 * nc) A.partials[((int64_t)blockIdx.x * A.n_list + c0) * 2 + threadIdx.x] = total;
}

struct TakeArgs {
    const void *plane;
    int64_t quads, quads_per_wg;
    void *core, *covered;
    uint64_t *partials;  // [grid.x][2]: core, covered
};

template <typename Cell>
__global__ __launch_bounds__(kThreads) void cover_take_kernel(const TakeArgs A) {
    using Sum = typename Quad<Cell>::Sum;
    const uint4 *plane = static_cast<const uint4 *>(A.plane);
    uint4 *core = static_cast<uint4 *>(A.core), *covered = static_cast<uint4 *>(A.covered);
    Sum acc[2] = {0, 0};
    const int64_t q0 = (int64_t)blockIdx.x * A.quads_per_wg, q1 = min(q0 + A.quads_per_wg, A.quads);
    for (int64_t q = q0 + threadIdx.x; q < q1; q += kThreads) {
        const uint4 p = plane[q];
        const uint4 keep = quad_min<Cell>(core[q], p), seen = quad_max<Cell>(covered[q], p);
        core[q] = keep;
        covered[q] = seen;
        acc[0] += quad_sum<Cell>(keep);
        acc[1] += quad_sum<Cell>(seen);
    }
    const uint64_t total = group_sums(acc);
    if (threadIdx.x < 2) A.partials[(int64_t)blockIdx.x * 2 + threadIdx.x] = total;
}

// one wave per cell: lane x sums the cell over every 64th workgroup of the sweep's grid.x, the wave adds the 64 sums up
__global__ __launch_bounds__(kThreads) void cover_reduce_kernel(const uint64_t *partials, int gx, int64_t cells, uint64_t *out) {
    const int64_t cell = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (cell >= cells) return;  // (whole waves)
    uint64_t sum = 0;
    for (int x = threadIdx.x & 63; x < gx; x += 64) sum += partials[(int64_t)x * cells + cell];
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0) out[cell] = sum;
}

inline bool misaligned(const void *p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) != 0; }

// the refusals every entry shares: the cell, the planes' pitch and base
int check_planes(const void *d_weights, int64_t pitch, int32_t cell_bytes) {
    if (cell_bytes != 2 && cell_bytes != 4) return fail(MEMO_EINVAL, "cell_bytes must be 2 or 4 (cell_bytes = %d)", cell_bytes);
    const int64_t quad = 16 / cell_bytes;
    if (pitch < quad || pitch % quad) return fail(MEMO_EINVAL, "pitch must be a positive multiple of %lld cells (pitch = %lld)", (long long)quad, (long long)pitch);
    if (!d_weights || misaligned(d_weights, 16)) return fail(MEMO_EINVAL, "d_weights is NULL or not 16-byte aligned");
    return MEMO_OK;
}

// ... and those of begin, score and take: how many planes, the cells read, the masks
int check_masks(const void *d_weights, int64_t pitch, int32_t num_planes, int32_t cell_bytes, int64_t cells, const void *d_core, const void *d_covered) {
    if (int rc = check_planes(d_weights, pitch, cell_bytes)) return rc;
    if (num_planes < 1 || num_planes > kMaxDocs) return fail(MEMO_EINVAL, "a cover is made for 1 to %d planes (num_planes = %d)", kMaxDocs, num_planes);
    if (cells < 0 || cells % (16 / cell_bytes) || cells > pitch)
        return fail(MEMO_EINVAL, "cells must be a multiple of %d in [0, pitch] (cells = %lld, pitch = %lld)", 16 / cell_bytes, (long long)cells, (long long)pitch);
    if (cells > (int64_t)kCapMax + 16) return fail(MEMO_EINVAL, "masks of %lld cells are too long", (long long)cells);
    if (!d_core || !d_covered || misaligned(d_core, 16) || misaligned(d_covered, 16)) return fail(MEMO_EINVAL, "d_core or d_covered is NULL or not 16-byte aligned");
    return MEMO_OK;
}

int check_span(uint32_t span, int32_t cell_bytes) {
    if (span < 1 || span > kCapMax) return fail(MEMO_EINVAL, "the span must be in [1, %u] (span = %u)", kCapMax, span);
    if (cell_bytes == 2 && span > 0xFFFFu) return fail(MEMO_EINVAL, "a span of %u does not fit cells of 2 bytes", span);
    return MEMO_OK;
}

// grid.x and the quads a workgroup takes, a multiple of kThreads; `most`: workgroups along the cells at most, unless the bound of the
// 2-byte lane sums needs more
void split_quads(int64_t quads, int64_t most, int32_t cell_bytes, int *gx, int64_t *per) {
    const int64_t passes = (quads + kThreads - 1) / kThreads;
    const int64_t need = cell_bytes == 2 ? (passes + kMaxPasses16 - 1) / kMaxPasses16 : 1;  // at most 128: cells <= 2^31 + 15
    const int64_t cap = std::max<int64_t>({(int64_t)1, std::min<int64_t>({most, passes, (int64_t)kMaxGridX}), need});
    *per = (passes + cap - 1) / cap * kThreads;
    *gx = (int)((quads + *per - 1) / *per);
}

}  // namespace

extern "C" {

int32_t memo_cover_pass_cells(int32_t cell_bytes) { return cell_bytes == 2 || cell_bytes == 4 ? kThreads * 16 / cell_bytes : 0; }

int memo_cover_weights_dev(const uint32_t *d_lengths, int64_t Ls, int64_t pitch_src, int32_t num_docs, uint32_t kmin, uint32_t kmax, const uint16_t *list_host,
                           int32_t n_list, void *d_weights, int64_t pitch, int32_t cell_bytes, int64_t cell0, int32_t device, void *stream) {
    if (num_docs < 1 || num_docs > kMaxDocs) return fail(MEMO_EINVAL, "lengths of 1 to %d genomes (num_docs = %d)", kMaxDocs, num_docs);
    if (n_list < 0 || n_list > kMaxList) return fail(MEMO_EINVAL, "n_list must be in [0, %d]", kMaxList);
    if (int rc = check_planes(d_weights, pitch, cell_bytes)) return rc;
    if (kmax < 1 || kmax > kCapMax || kmin < 1 || kmin > kmax)
        return fail(MEMO_EINVAL, "kmin and kmax must hold 1 <= kmin <= kmax <= %u (kmin = %u, kmax = %u)", kCapMax, kmin, kmax);
    if (int rc = check_span(kmax - kmin + 1, cell_bytes)) return rc;
    if (Ls < 0 || (Ls && !d_lengths)) return fail(MEMO_EINVAL, "bad lengths (Ls = %lld)", (long long)Ls);
    if (misaligned(d_lengths, 16)) return fail(MEMO_EINVAL, "d_lengths must be 16-byte aligned");
    if (pitch_src < Ls || (pitch_src & 3)) return fail(MEMO_EINVAL, "pitch_src must be a multiple of 4 and at least Ls (pitch_src = %lld, Ls = %lld)", (long long)pitch_src, (long long)Ls);
    if (cell0 < 0 || (cell0 & 7) || cell0 > pitch || Ls > pitch - cell0)
        return fail(MEMO_EINVAL, "cells [%lld, %lld) leave a plane of %lld cells, or do not begin at a multiple of 8", (long long)cell0, (long long)(cell0 + Ls), (long long)pitch);
    if (n_list && !list_host) return fail(MEMO_EINVAL, "the list is NULL");
    for (int i = 0; i < n_list; ++i)
        if (list_host[i] >= num_docs) return fail(MEMO_EINVAL, "entry %d of the list: genome %d of %d", i, (int)list_host[i], num_docs);
    if (!Ls || !n_list) return MEMO_OK;
    const int64_t quad = 16 / cell_bytes, groups = ((Ls + quad - 1) / quad + kThreads - 1) / kThreads;
    if (groups > INT32_MAX) return fail(MEMO_EINVAL, "a slice of %lld positions is too long", (long long)Ls);

    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DevPtr<uint16_t> d_list;
    if (hipError_t err = d_list.alloc((size_t)n_list); err != hipSuccess)
        return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the list of %d genomes: %s", (size_t)n_list * sizeof(uint16_t), n_list, hipGetErrorString(err));
    HIP_TRY(hipMemcpyAsync(d_list, list_host, (size_t)n_list * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    WeightsArgs A = {};
    A.lengths = d_lengths;
    A.Ls = Ls;
    A.pitch_src = pitch_src;
    A.kmin = kmin;
    A.kmax = kmax;
    A.list = d_list;
    A.weights = d_weights;
    A.pitch = pitch;
    A.cell0 = cell0;
    Laps laps(st, g_cover_timed, g_cover_ms);
    if (int rc = laps.start()) return rc;
    const dim3 grid((unsigned)groups, (unsigned)n_list);
    if (cell_bytes == 2)
        hipLaunchKernelGGL(cover_weights_kernel<uint16_t>, grid, dim3(kThreads), 0, st, A);
    else
        hipLaunchKernelGGL(cover_weights_kernel<uint32_t>, grid, dim3(kThreads), 0, st, A);
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(0)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return MEMO_OK;
}

int memo_cover_begin_dev(void *d_weights, int64_t pitch, int32_t num_planes, int32_t cell_bytes, int64_t L, uint32_t span, void *d_core, void *d_covered,
                         int32_t device, void *stream) {
    if (L < 0) return fail(MEMO_EINVAL, "bad window (L = %lld)", (long long)L);
    if (int rc = check_planes(d_weights, pitch, cell_bytes)) return rc;
    const int64_t quad = 16 / cell_bytes, cells = (L + quad - 1) / quad * quad;
    if (int rc = check_masks(d_weights, pitch, num_planes, cell_bytes, std::min(cells, pitch), d_core, d_covered)) return rc;
    if (cells > pitch) return fail(MEMO_EINVAL, "a window of %lld positions needs planes of %lld cells (pitch = %lld)", (long long)L, (long long)cells, (long long)pitch);
    if (int rc = check_span(span, cell_bytes)) return rc;
    if (!L) return MEMO_OK;
    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t items = std::max<int64_t>(cells, (quad - 1) * num_planes);
    const dim3 grid((unsigned)((items + kThreads - 1) / kThreads));
    if (cell_bytes == 2)
        hipLaunchKernelGGL(cover_begin_kernel<uint16_t>, grid, dim3(kThreads), 0, st, static_cast<uint16_t *>(d_weights), pitch, (int)num_planes, L, span,
                           static_cast<uint16_t *>(d_core), static_cast<uint16_t *>(d_covered));
    else
        hipLaunchKernelGGL(cover_begin_kernel<uint32_t>, grid, dim3(kThreads), 0, st, static_cast<uint32_t *>(d_weights), pitch, (int)num_planes, L, span,
                           static_cast<uint32_t *>(d_core), static_cast<uint32_t *>(d_covered));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return MEMO_OK;
}

int memo_cover_score_dev(const void *d_weights, int64_t pitch, int32_t num_planes, int32_t cell_bytes, int64_t cells, const void *d_core, const void *d_covered,
                         const uint16_t *list_host, int32_t n_list, uint64_t *scores_host, int32_t device, void *stream) {
    if (int rc = check_masks(d_weights, pitch, num_planes, cell_bytes, cells, d_core, d_covered)) return rc;
    if (n_list < 0 || n_list > kMaxList) return fail(MEMO_EINVAL, "n_list must be in [0, %d]", kMaxList);
    if (n_list && (!list_host || !scores_host)) return fail(MEMO_EINVAL, "the list or the scores are NULL");
    for (int i = 0; i < n_list; ++i)
        if (list_host[i] >= num_planes) return fail(MEMO_EINVAL, "entry %d of the list: plane %d of %d", i, (int)list_host[i], num_planes);
    if (!n_list) return MEMO_OK;
    if (!cells) {
        memset(scores_host, 0, (size_t)n_list * 2 * sizeof(uint64_t));
        return MEMO_OK;
    }
    ScoreArgs A = {};
    A.weights = d_weights;
    A.pitch = pitch;
    A.quads = cells / (16 / cell_bytes);
    A.core = d_core;
    A.covered = d_covered;
    A.n_list = n_list;
    const int gy = (n_list + kBlock - 1) / kBlock;
    const size_t row_bytes = (size_t)n_list * 2 * sizeof(uint64_t);  // of the partials, per workgroup along the cells
    int gx = 0;
    split_quads(A.quads, std::min<int64_t>(std::max(1, kTargetGroups / gy), (int64_t)(kScratchCap / row_bytes)), cell_bytes, &gx, &A.quads_per_wg);

    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // one allocation: the 64-bit results, the partials, and behind them the list
    DevPtr<uint64_t> scratch;
    const size_t out_n = (size_t)n_list * 2, part_n = (size_t)gx * n_list * 2, total_n = out_n + part_n + ((size_t)n_list + 3) / 4;
    if (hipError_t err = scratch.alloc(total_n); err != hipSuccess)
        return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the partial scores of %d planes and the list: %s", total_n * sizeof(uint64_t), n_list, hipGetErrorString(err));
    uint64_t *d_out = scratch.p;
    A.partials = scratch + out_n;
    uint16_t *d_list = reinterpret_cast<uint16_t *>(scratch + out_n + part_n);
    HIP_TRY(hipMemcpyAsync(d_list, list_host, (size_t)n_list * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    A.list = d_list;
    Laps laps(st, g_cover_timed, g_cover_ms);
    if (int rc = laps.start()) return rc;
    const dim3 grid((unsigned)gx, (unsigned)gy);
    if (cell_bytes == 2)
        hipLaunchKernelGGL(cover_score_kernel<uint16_t>, grid, dim3(kThreads), 0, st, A);
    else
        hipLaunchKernelGGL(cover_score_kernel<uint32_t>, grid, dim3(kThreads), 0, st, A);
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(1)) return rc;
    const int64_t sums = (int64_t)n_list * 2;
    hipLaunchKernelGGL(cover_reduce_kernel, dim3((unsigned)((sums + kThreads / 64 - 1) / (kThreads / 64))), dim3(kThreads), 0, st, A.partials, gx, sums, d_out);
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(2)) return rc;
    HIP_TRY(hipMemcpyAsync(scores_host, d_out, (size_t)sums * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MEMO_OK;
}

int memo_cover_take_dev(const void *d_weights, int64_t pitch, int32_t num_planes, int32_t cell_bytes, int64_t cells, int32_t plane, void *d_core, void *d_covered,
                        uint64_t *sums_host, int32_t device, void *stream) {
    if (int rc = check_masks(d_weights, pitch, num_planes, cell_bytes, cells, d_core, d_covered)) return rc;
    if (plane < 0 || plane >= num_planes) return fail(MEMO_EINVAL, "plane %d of %d", plane, num_planes);
    if (!sums_host) return fail(MEMO_EINVAL, "the sums are NULL");
    if (!cells) {
        sums_host[0] = sums_host[1] = 0;
        return MEMO_OK;
    }
    TakeArgs A = {};
    A.plane = static_cast<const char *>(d_weights) + (int64_t)plane * pitch * cell_bytes;
    A.quads = cells / (16 / cell_bytes);
    A.core = d_core;
    A.covered = d_covered;
    int gx = 0;
    split_quads(A.quads, kMaxGridX, cell_bytes, &gx, &A.quads_per_wg);

    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DevPtr<uint64_t> scratch;  // the two 64-bit sums, then the partials
    const size_t total_n = 2 + (size_t)gx * 2;
    if (hipError_t err = scratch.alloc(total_n); err != hipSuccess)
        return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the partial sums of a step: %s", total_n * sizeof(uint64_t), hipGetErrorString(err));
    uint64_t *d_out = scratch.p;
    A.partials = scratch + 2;
    Laps laps(st, g_cover_timed, g_cover_ms);
    if (int rc = laps.start()) return rc;
    if (cell_bytes == 2)
        hipLaunchKernelGGL(cover_take_kernel<uint16_t>, dim3((unsigned)gx), dim3(kThreads), 0, st, A);
    else
        hipLaunchKernelGGL(cover_take_kernel<uint32_t>, dim3((unsigned)gx), dim3(kThreads), 0, st, A);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(cover_reduce_kernel, dim3(1), dim3(kThreads), 0, st, A.partials, gx, (int64_t)2, d_out);
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(3)) return rc;
    HIP_TRY(hipMemcpyAsync(sums_host, d_out, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MEMO_OK;
}

}  // extern "C"
