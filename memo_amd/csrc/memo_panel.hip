// memo_panel.hip -- `memo panel`: the greedy set cover of a membership window's bits, one step at a time, on rows that stay in HBM as
// genome-major bit planes.  Plane g is pitch_words uint32 at d_planes + g * pitch_words; bit p & 31 of its word p >> 5 is the
// membership bit of genome g at window position p.  No counterpart in the reference.  The third reduction over positions after
// memo_cooc.hip and memo_collect.hip: those fold every slice where it lies and forget it; the greedy's every step depends on all the
// steps before it over the whole window, so here the slices are kept, transposed (memo_planes.h), and a step is a stream over them.
//
//   memo_panel_planes_dev   one slice's rows uint32 [L][W] -> words [word0, word0 + ceil(L / 32)) of every plane.  One tile = kTileWords
//       = 32 plane words (1024 positions), aligned to the PLANE's words (a tile starts at a multiple of 4 words of the plane, so
//       that word0 = 1 or 5 still leaves 16-byte stores aligned), by kChunk = 8 genome words (256 genomes): a workgroup of 256 lanes
//       stages its 32 x 8 blocks, one a lane (stage_plane_block: one load per row word, rows at or past L as zeros, bits at or above
//       num_docs masked, transpose32, 16-byte stores into LDS at the 36-word pitch), and after one barrier writes them out genome by
//       genome: eight lanes a genome, 16 bytes a lane, 128 contiguous bytes a plane.  A quad that lies whole inside the slice's words
//       leaves as one 16-byte store, one that straddles an end word by word; nothing outside the slice's words is written.
//   memo_panel_begin_dev    what no slice writes: the pad words [ceil(L / 32), the next multiple of 4) of every plane as zeros, core
//       as ones below L (zeros in the last word's tail and in the pad), covered as zeros.
//   memo_panel_score_dev    for a host list of genome ids g (repeats are legal): new = |plane g & ~covered|, kept = |plane g & core|.
//       A streaming kernel: a workgroup takes a span of the words (grid.x) and a block of kBlock = 8 candidates (grid.y); a lane
//       reads 16 bytes of each mask once per block and 16 bytes of each of the block's planes, and adds v_bcnt of plane & ~covered
//       and of plane & core to 16 register accumulators (a block's tail repeats its first candidate; those sums never leave).  Then
//       a wave reduce (DPP inside rows of 16, two shuffles across them), the four waves through LDS, and 32-bit partials
//       [grid.x][n_list][2]; panel_reduce_kernel sums them over grid.x in 64 bits, one wave a cell.
//   memo_panel_take_dev     core &= plane g, covered |= plane g in place (a quad is read and written by one lane), and the two new
//       counts by the same partials and reduce launch.
//
// Conditions the code holds:
//   - no workgroup waits for another: no look-back, no flag in memory, no cooperative launch
//   - no global atomics: every partial and every output cell has one owner, and the stream orders the launches
//   - planes_dev reads nothing outside d_bits[0 .. L * W) and writes nothing outside words [word0, word0 + ceil(L / 32)) of the planes
//     [0, num_docs); score and take read words [0, words) of a plane and of the masks, words a multiple of 4 and at most pitch_words
//   - MEMO_EINVAL before any launch leaves planes, masks and outputs as they were: a base that is not 16-byte aligned, a pitch that is
//     no multiple of 4, a range that leaves the pitch, a genome id at or above num_docs, num_docs outside [1, 2048]
//   - the 32-bit partials cannot wrap: a workgroup takes at most 2^26 words (2^31 bits); longer masks are refused
//   - scratch: the partials (at most 64 MiB: grid.x gives way), the uploaded list and the 64-bit results, one allocation that DevPtr
//     owns; an allocation that fails is MEMO_EHIP with the bytes asked for, and nothing stays allocated
//   - vector loads and stores and plain C++ only
#include <algorithm>

#include "memo_planes.h"

using namespace memo;

namespace memo {
thread_local int g_panel_timed = 0;  // 1 = event pairs around the launches (memo_debug_panel_times), each launch waited for
thread_local float g_panel_ms[4] = {0.f, 0.f, 0.f, 0.f};  // ... of the last such call of each kind: planes, the score sweep, its reduce, take
}

namespace {

constexpr int kThreads = 256;
constexpr int kMaxDocs = 2048;
constexpr int kTileWords = 32;                 // plane words a tile of memo_panel_planes_dev: 128 bytes a plane
constexpr int kChunk = 8;                      // genome words a workgroup of it stages: 32 x 8 blocks, one a lane
constexpr int kChunkPitch = kPlaneBlockPitch * kChunk + 4;  // LDS words per plane word of the tile
constexpr int kBlock = 8;                      // candidates a workgroup of the score kernel takes
constexpr int kPassWords = 4 * kThreads;       // mask words a workgroup takes per pass: 16 bytes a lane
constexpr int64_t kMaxQuadsPerWg = (int64_t)1 << 24;  // x 128 bits = 2^31: what keeps the 32-bit partials exact
constexpr int kTargetGroups = 2048;            // workgroups a score launch aims at: eight a CU
constexpr int kMaxGridX = 2048;
constexpr size_t kScratchCap = (size_t)64 << 20;
constexpr int kMaxList = 65535;

// ------------------------------------------------------------------------------------------------------------------------------
// rows -> planes
// ------------------------------------------------------------------------------------------------------------------------------
struct PlanesArgs {
    const uint32_t *bits;
    int64_t L, nw;       // the slice's positions, its plane words
    int W, N;
    uint32_t *planes;
    int64_t pitch, word0;
    int shift;           // word0 & 3: tile t holds the plane words word0 - shift + 32 t ...
};

__global__ __launch_bounds__(kThreads) void panel_planes_kernel(const PlanesArgs A) {
    __shared__ __attribute__((aligned(16))) uint32_t planes[kTileWords * kChunkPitch];
    const int w0 = blockIdx.y * kChunk;
    const int64_t s0 = (int64_t)blockIdx.x * kTileWords - A.shift;  // the slice word of the tile's first plane word (below 0: before the slice)
    {
        const int w = w0 + (int)(threadIdx.x % kChunk), P = threadIdx.x / kChunk;
        const int64_t sw = s0 + P;
        if (w < A.W && sw >= 0 && sw < A.nw) stage_plane_block(A.bits, A.L, A.W, A.N, w, 32 * sw, planes + P * kChunkPitch + kPlaneBlockPitch * (w - w0));
    }
    __syncthreads();
    const int quad = threadIdx.x % 8;
    const int64_t sq = s0 + 4 * quad;  // the slice word of the quad's first word
    if (sq + 4 <= 0 || sq >= A.nw) return;
    const bool whole = sq >= 0 && sq + 4 <= A.nw;
    for (int gl = threadIdx.x / 8; gl < 32 * kChunk; gl += kThreads / 8) {
        const int g = 32 * w0 + gl;
        if (g >= A.N) break;
        const uint32_t *src = planes + (4 * quad) * kChunkPitch + kPlaneBlockPitch * (gl >> 5) + (gl & 31);
        uint32_t *dst = A.planes + (int64_t)g * A.pitch + A.word0 + sq;
        const uint32_t v[4] = {src[0], src[kChunkPitch], src[2 * kChunkPitch], src[3 * kChunkPitch]};
        if (whole) {
            *reinterpret_cast<uint4 *>(dst) = make_uint4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (sq + i >= 0 && sq + i < A.nw) dst[i] = v[i];
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// the pads and the masks
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void panel_begin_kernel(uint32_t *planes, int64_t pitch, int N, int64_t L, uint32_t *core, uint32_t *covered) {
    const int64_t nw = (L + 31) / 32, nw4 = (nw + 3) & ~(int64_t)3;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < nw4) {
        core[i] = i < L / 32 ? 0xFFFFFFFFu : i < nw ? (1u << (L & 31)) - 1u : 0u;
        covered[i] = 0u;
    }
    const int64_t pad = nw4 - nw;  // 0 .. 3 words a plane
    if (i < pad * N) planes[(i / pad) * pitch + nw + i % pad] = 0u;
}

// ------------------------------------------------------------------------------------------------------------------------------
// score, take, and the reduce launch behind both
// ------------------------------------------------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_add(uint32_t v) {
    return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}

// the sum of v over the wave's 64 lanes, in every one of them
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    v = dpp_add<0xB1>(v);   // quad_perm [1, 0, 3, 2]: lane ^ 1
    v = dpp_add<0x4E>(v);   // quad_perm [2, 3, 0, 1]: lane ^ 2
    v = dpp_add<0x141>(v);  // row_half_mirror: the other quad's sum
    v = dpp_add<0x140>(v);  // row_mirror: the other half's sum
    v += (uint32_t)__shfl_xor((int)v, 16);
    v += (uint32_t)__shfl_xor((int)v, 32);
    return v;
}

__device__ __forceinline__ uint32_t popc4(const uint4 p, const uint4 m) {
    return (uint32_t)(__popc(p.x & m.x) + __popc(p.y & m.y) + __popc(p.z & m.z) + __popc(p.w & m.w));
}

struct ScoreArgs {
    const uint32_t *planes;
    int64_t pitch;
    int64_t quads, quads_per_wg;  // 16-byte quads of the masks, and of one workgroup's span (a multiple of kThreads)
    const uint32_t *core, *covered;
    const uint16_t *list;         // [n_list], on the device
    int n_list;
    uint32_t *partials;           // [grid.x][n_list][2]: new, kept
};

// the workgroup's sums of VALUES values a lane: out[i] in lanes 0 .. VALUES - 1 of the workgroup's first wave (tid = i) on return
template <int VALUES>
__device__ __forceinline__ uint32_t group_sums(uint32_t (&acc)[VALUES]) {
    __shared__ uint32_t wsum[kThreads / 64][VALUES];
#pragma unroll
    for (int i = 0; i < VALUES; ++i) acc[i] = wave_sum(acc[i]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < VALUES; ++i) wsum[threadIdx.x >> 6][i] = acc[i];
    }
    __syncthreads();
    uint32_t total = 0;
    if (threadIdx.x < VALUES)
        for (int wv = 0; wv < kThreads / 64; ++wv) total += wsum[wv][threadIdx.x];
    return total;
}

__global__ __launch_bounds__(kThreads) void panel_score_kernel(const ScoreArgs A) {
    const int c0 = blockIdx.y * kBlock, nc = min(kBlock, A.n_list - c0);
    const uint4 *plane[kBlock];
#pragma unroll
    for (int c = 0; c < kBlock; ++c)
        plane[c] = reinterpret_cast<const uint4 *>(A.planes + (int64_t)A.list[c0 + (c < nc ? c : 0)] * A.pitch);
    const uint4 *core = reinterpret_cast<const uint4 *>(A.core), *covered = reinterpret_cast<const uint4 *>(A.covered);
    uint32_t acc[2 * kBlock] = {};
    const int64_t q0 = (int64_t)blockIdx.x * A.quads_per_wg, q1 = min(q0 + A.quads_per_wg, A.quads);
    for (int64_t q = q0 + threadIdx.x; q < q1; q += kThreads) {
        const uint4 keep = core[q], seen = covered[q];
        const uint4 fresh = make_uint4(~seen.x, ~seen.y, ~seen.z, ~seen.w);
        uint4 p[kBlock];
#pragma unroll
        for (int c = 0; c < kBlock; ++c) p[c] = plane[c][q];
#pragma unroll
        for (int c = 0; c < kBlock; ++c) {
            acc[2 * c] += popc4(p[c], fresh);
            acc[2 * c + 1] += popc4(p[c], keep);
        }
    }
    const uint32_t total = group_sums(acc);
    if ((int)threadIdx.x < 2 * nc) A.partials[((int64_t)blockIdx.x * A.n_list + c0) * 2 + threadIdx.x] = total;
}

struct TakeArgs {
    const uint32_t *plane;
    int64_t quads, quads_per_wg;
    uint32_t *core, *covered;
    uint32_t *partials;  // [grid.x][2]: core, covered
};

__global__ __launch_bounds__(kThreads) void panel_take_kernel(const TakeArgs A) {
    const uint4 *plane = reinterpret_cast<const uint4 *>(A.plane);
    uint4 *core = reinterpret_cast<uint4 *>(A.core), *covered = reinterpret_cast<uint4 *>(A.covered);
    uint32_t acc[2] = {0u, 0u};
    const uint4 ones = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
    const int64_t q0 = (int64_t)blockIdx.x * A.quads_per_wg, q1 = min(q0 + A.quads_per_wg, A.quads);
    for (int64_t q = q0 + threadIdx.x; q < q1; q += kThreads) {
        const uint4 p = plane[q];
        uint4 keep = core[q], seen = covered[q];
        keep = make_uint4(keep.x & p.x, keep.y & p.y, keep.z & p.z, keep.w & p.w);
        seen = make_uint4(seen.x | p.x, seen.y | p.y, seen.z | p.z, seen.w | p.w);
        core[q] = keep;
        covered[q] = seen;
        acc[0] += popc4(keep, ones);
        acc[1] += popc4(seen, ones);
    }
    const uint32_t total = group_sums(acc);
    if (threadIdx.x < 2) A.partials[(int64_t)blockIdx.x * 2 + threadIdx.x] = total;
}

// one wave per cell: lane x sums the cell over every 64th workgroup of the sweep's grid.x, the wave adds the 64 sums up in two halves
__global__ __launch_bounds__(kThreads) void panel_reduce_kernel(const uint32_t *partials, int gx, int64_t cells, uint64_t *out) {
    const int64_t cell = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (cell >= cells) return;  // (whole waves)
    uint64_t sum = 0;
    for (int x = threadIdx.x & 63; x < gx; x += 64) sum += partials[(int64_t)x * cells + cell];
    uint32_t lo = (uint32_t)sum, hi = (uint32_t)(sum >> 32);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const uint32_t lo2 = (uint32_t)__shfl_xor((int)lo, m), hi2 = (uint32_t)__shfl_xor((int)hi, m);
        const uint64_t both = ((uint64_t)hi << 32 | lo) + ((uint64_t)hi2 << 32 | lo2);
        lo = (uint32_t)both;
        hi = (uint32_t)(both >> 32);
    }
    if ((threadIdx.x & 63) == 0) out[cell] = (uint64_t)hi << 32 | lo;
}

inline bool misaligned(const void *p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) != 0; }

// the refusals score and take share
int check_planes(const uint32_t *d_planes, int64_t pitch_words, int32_t num_docs, int64_t words, const uint32_t *d_core, const uint32_t *d_covered) {
    if (num_docs < 1 || num_docs > kMaxDocs) return fail(MEMO_EINVAL, "a panel is made for 1 to %d genomes (num_docs = %d)", kMaxDocs, num_docs);
    if (pitch_words < 4 || (pitch_words & 3)) return fail(MEMO_EINVAL, "pitch_words must be a positive multiple of 4 (pitch_words = %lld)", (long long)pitch_words);
    if (!d_planes || misaligned(d_planes, 16)) return fail(MEMO_EINVAL, "d_planes is NULL or not 16-byte aligned");
    if (words < 0 || (words & 3) || words > pitch_words)
        return fail(MEMO_EINVAL, "words must be a multiple of 4 in [0, pitch_words] (words = %lld, pitch_words = %lld)", (long long)words, (long long)pitch_words);
    if (!d_core || !d_covered || misaligned(d_core, 16) || misaligned(d_covered, 16)) return fail(MEMO_EINVAL, "d_core or d_covered is NULL or not 16-byte aligned");
    return MEMO_OK;
}

// grid.x and the quads a workgroup takes, a multiple of kThreads; `most`: workgroups along the words at most
int split_quads(int64_t quads, int64_t most, int *gx, int64_t *per) {
    const int64_t passes = (quads + kThreads - 1) / kThreads;
    const int64_t cap = std::max<int64_t>(1, std::min<int64_t>({most, passes, (int64_t)kMaxGridX}));
    *per = (passes + cap - 1) / cap * kThreads;
    if (*per > kMaxQuadsPerWg) return fail(MEMO_EINVAL, "masks of %lld words are too long", (long long)(4 * quads));
    *gx = (int)((quads + *per - 1) / *per);
    return MEMO_OK;
}

}  // namespace

extern "C" {

int32_t memo_panel_tile(void) { return 32 * kTileWords; }
int32_t memo_panel_pass_words(void) { return kPassWords; }

int memo_panel_planes_dev(const uint32_t *d_bits, int64_t L, int32_t num_docs, uint32_t *d_planes, int64_t pitch_words, int64_t word0, int32_t device,
                          void *stream) {
    if (num_docs < 1 || num_docs > kMaxDocs) return fail(MEMO_EINVAL, "a panel is made for 1 to %d genomes (num_docs = %d)", kMaxDocs, num_docs);
    if (L < 0 || (L && !d_bits)) return fail(MEMO_EINVAL, "bad membership result (L = %lld)", (long long)L);
    if (misaligned(d_bits, 16)) return fail(MEMO_EINVAL, "d_bits must be 16-byte aligned");
    if (pitch_words < 4 || (pitch_words & 3)) return fail(MEMO_EINVAL, "pitch_words must be a positive multiple of 4 (pitch_words = %lld)", (long long)pitch_words);
    if (!d_planes || misaligned(d_planes, 16)) return fail(MEMO_EINVAL, "d_planes is NULL or not 16-byte aligned");
    const int64_t nw = (L + 31) / 32;
    if (word0 < 0 || word0 > pitch_words || nw > pitch_words - word0)
        return fail(MEMO_EINVAL, "words [%lld, %lld) leave a plane of %lld words", (long long)word0, (long long)(word0 + nw), (long long)pitch_words);
    if (!L) return MEMO_OK;
    PlanesArgs A = {};
    A.bits = d_bits;
    A.L = L;
    A.nw = nw;
    A.W = (num_docs + 31) / 32;
    A.N = num_docs;
    A.planes = d_planes;
    A.pitch = pitch_words;
    A.word0 = word0;
    A.shift = (int)(word0 & 3);
    const int64_t tiles = (nw + A.shift + kTileWords - 1) / kTileWords;
    if (tiles > INT32_MAX) return fail(MEMO_EINVAL, "a slice of %lld positions is too long", (long long)L);
    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Laps laps(st, g_panel_timed, g_panel_ms);
    if (int rc = laps.start()) return rc;
    hipLaunchKernelGGL(panel_planes_kernel, dim3((unsigned)tiles, (unsigned)((A.W + kChunk - 1) / kChunk)), dim3(kThreads), 0, st, A);
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(0)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return MEMO_OK;
}

int memo_panel_begin_dev(uint32_t *d_planes, int64_t pitch_words, int32_t num_docs, int64_t L, uint32_t *d_core, uint32_t *d_covered, int32_t device,
                         void *stream) {
    if (L < 0) return fail(MEMO_EINVAL, "bad window (L = %lld)", (long long)L);
    const int64_t nw4 = ((L + 31) / 32 + 3) & ~(int64_t)3;
    if (int rc = check_planes(d_planes, pitch_words, num_docs, std::min(nw4, pitch_words), d_core, d_covered)) return rc;
    if (nw4 > pitch_words) return fail(MEMO_EINVAL, "a window of %lld positions needs planes of %lld words (pitch_words = %lld)", (long long)L, (long long)nw4, (long long)pitch_words);
    if (!L) return MEMO_OK;
    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t items = std::max<int64_t>(nw4, (int64_t)3 * num_docs);
    hipLaunchKernelGGL(panel_begin_kernel, dim3((unsigned)((items + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, d_planes, pitch_words, (int)num_docs, L,
                       d_core, d_covered);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return MEMO_OK;
}

int memo_panel_score_dev(const uint32_t *d_planes, int64_t pitch_words, int32_t num_docs, int64_t words, const uint32_t *d_core, const uint32_t *d_covered,
                         const uint16_t *list_host, int32_t n_list, uint64_t *scores_host, int32_t device, void *stream) {
    if (int rc = check_planes(d_planes, pitch_words, num_docs, words, d_core, d_covered)) return rc;
    if (n_list < 0 || n_list > kMaxList) return fail(MEMO_EINVAL, "n_list must be in [0, %d]", kMaxList);
    if (n_list && (!list_host || !scores_host)) return fail(MEMO_EINVAL, "the list or the scores are NULL");
    for (int i = 0; i < n_list; ++i)
        if (list_host[i] >= num_docs) return fail(MEMO_EINVAL, "entry %d of the list: genome %d of %d", i, (int)list_host[i], num_docs);
    if (!n_list) return MEMO_OK;
    if (!words) {
        memset(scores_host, 0, (size_t)n_list * 2 * sizeof(uint64_t));
        return MEMO_OK;
    }
    ScoreArgs A = {};
    A.planes = d_planes;
    A.pitch = pitch_words;
    A.quads = words / 4;
    A.core = d_core;
    A.covered = d_covered;
    A.n_list = n_list;
    const int gy = (n_list + kBlock - 1) / kBlock;
    const size_t cell_bytes = (size_t)n_list * 2 * sizeof(uint32_t);
    int gx = 0;
    if (int rc = split_quads(A.quads, std::min<int64_t>(std::max(1, kTargetGroups / gy), (int64_t)(kScratchCap / cell_bytes)), &gx, &A.quads_per_wg)) return rc;

    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // one allocation: the 64-bit results, the partials, and behind them the list
    DevPtr<uint32_t> scratch;
    const size_t out_n = (size_t)n_list * 4, part_n = (size_t)gx * n_list * 2, words_n = out_n + part_n + ((size_t)n_list + 1) / 2;
    if (hipError_t err = scratch.alloc(words_n); err != hipSuccess)
        return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the partial scores of %d genomes and the list: %s", words_n * sizeof(uint32_t), n_list, hipGetErrorString(err));
    uint64_t *d_out = reinterpret_cast<uint64_t *>(scratch.p);
    A.partials = scratch + out_n;
    uint16_t *d_list = reinterpret_cast<uint16_t *>(scratch + out_n + part_n);
    HIP_TRY(hipMemcpyAsync(d_list, list_host, (size_t)n_list * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    A.list = d_list;
    Laps laps(st, g_panel_timed, g_panel_ms);
    if (int rc = laps.start()) return rc;
    hipLaunchKernelGGL(panel_score_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(kThreads), 0, st, A);
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(1)) return rc;
    const int64_t cells = (int64_t)n_list * 2;
    hipLaunchKernelGGL(panel_reduce_kernel, dim3((unsigned)((cells + kThreads / 64 - 1) / (kThreads / 64))), dim3(kThreads), 0, st, A.partials, gx, cells, d_out);
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(2)) return rc;
    HIP_TRY(hipMemcpyAsync(scores_host, d_out, (size_t)cells * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MEMO_OK;
}

int memo_panel_take_dev(const uint32_t *d_planes, int64_t pitch_words, int32_t num_docs, int64_t words, int32_t genome, uint32_t *d_core, uint32_t *d_covered,
                        uint64_t *counts_host, int32_t device, void *stream) {
    if (int rc = check_planes(d_planes, pitch_words, num_docs, words, d_core, d_covered)) return rc;
    if (genome < 0 || genome >= num_docs) return fail(MEMO_EINVAL, "genome %d of %d", genome, num_docs);
    if (!counts_host) return fail(MEMO_EINVAL, "the counts are NULL");
    if (!words) {
        counts_host[0] = counts_host[1] = 0;
        return MEMO_OK;
    }
    TakeArgs A = {};
    A.plane = d_planes + (int64_t)genome * pitch_words;
    A.quads = words / 4;
    A.core = d_core;
    A.covered = d_covered;
    int gx = 0;
    if (int rc = split_quads(A.quads, kMaxGridX, &gx, &A.quads_per_wg)) return rc;

    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DevPtr<uint32_t> scratch;  // the two 64-bit counts, then the partials
    const size_t words_n = 4 + (size_t)gx * 2;
    if (hipError_t err = scratch.alloc(words_n); err != hipSuccess)
        return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the partial counts of a step: %s", words_n * sizeof(uint32_t), hipGetErrorString(err));
    uint64_t *d_out = reinterpret_cast<uint64_t *>(scratch.p);
    A.partials = scratch + 4;
    Laps laps(st, g_panel_timed, g_panel_ms);
    if (int rc = laps.start()) return rc;
    hipLaunchKernelGGL(panel_take_kernel, dim3((unsigned)gx), dim3(kThreads), 0, st, A);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(panel_reduce_kernel, dim3(1), dim3(kThreads), 0, st, A.partials, gx, (int64_t)2, d_out);
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(3)) return rc;
    HIP_TRY(hipMemcpyAsync(counts_host, d_out, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MEMO_OK;
}

}  // extern "C"
