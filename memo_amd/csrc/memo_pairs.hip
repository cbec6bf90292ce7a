// memo_pairs.hip -- `memo pairs`: the k-free pairwise summary of a membership index, from the finished lengths of `memo lengths`
// that are still in HBM.  With w[g][p] = max(0, min(v[g][p], kmax) - (kmin - 1)), the number of k in [kmin, kmax] at which genome g
// holds the pivot's k-mer at p,
//     S[g][h] += sum over p in [0, L) of min(w[g][p], w[h][p])                    0 <= g, h < planes, uint64, symmetric
// which is `memo matrix -k k`'s matrix added up over every k of [kmin, kmax]: a Gram matrix under (min, +).  planes x planes integers
// and not planes x L lengths leave the device.  No counterpart in the reference, and no MFMA form: the work is one v_min_u32 and one
// add per pair and position, so the kernel is bound by vector issue and by how many LDS bytes feed an instruction, not by HBM.
//
// The cells are uint32 [planes][pitch], L of them per plane read: memo_lengths_finish_dev's layout, no halo.  A cell above kmax is
// clamped (a finished plane is not trusted to be capped); the clamp and the subtraction are monotone, so they commute with the
// minimum and are applied once per loaded cell, on the way into LDS, not per pair.
//
// Pair space (memo_cooc.hip's, with wider groups).  Genomes come in groups of eight; a UNIT is a pair of groups (a, b), an 8 x 8 block
// of genome pairs whose 64 accumulators live in one lane.  Only units with a <= b exist (the upper triangle; the mirror is written
// when the sums leave), numbered b (b + 1) / 2 + a.  A workgroup of 256 lanes owns 64 consecutive units: grid.y walks the units
// (large N costs workgroups, not registers), grid.x runs of consecutive tiles.  A wave's lanes are unit slots x POSITION SLOTS: with
// more than 32 units in the workgroup a lane a unit and one slot, with 32, 16 or 8 and fewer 2, 4 or 8 slots that take different
// quads of the tile, so that a workgroup of few units (few genomes, or the last of a pair space) still has work for its lanes; the
// four waves split the quads between them in the same way.
// 8 x 8 and not 4 x 4: per four positions a unit makes sixteen 16-byte LDS reads (4 LDS clocks a wave each) for 256 minima and, as
// compiled, 128 three-operand adds (2 issue clocks a wave each); the CU's four SIMDs share one LDS, which that keeps busy a third of
// the time where 4 x 4 (eight reads for 64 + 32 instructions) keeps it busy two thirds.
// At most 128 genomes are staged by a launch; more are cut into chunks of 64, one launch per pair of chunks (ca <= cb) that stages
// both; ca < cb is a full rectangle of units, not a triangle.  Right for every planes in [1, 2048], made to be fast up to a few hundred.
//
// One tile = 128 positions = 32 quads of four.  Per tile a workgroup
//   1. stages: one lane per (staged genome, quad) makes one 16-byte load -- cell by cell where the load would cross L --, turns the
//      four cells into weights and writes them to LDS with one 16-byte store.  LDS is uint4 [staged genome][32 quads], the quads of a
//      genome rotated by its group's number: the lanes of a wave read the same quad of different groups, which would otherwise all
//      fall on the same banks.  Genomes at or past `planes` in a padded group and positions at or past L are zeros.  A triangle
//      workgroup stages only the groups up to the largest b of its units.
//   2. accumulates: per quad and unit eight 16-byte reads (group a), then for each genome of group b one 16-byte read -- issued
//      under the genome before -- and 8 x 4 x (v_min_u32, add).
// Accumulator width.  w <= span = kmax - kmin + 1.
//   narrow (span x tile < 2^32)   32-bit accumulators, which cannot wrap inside one tile; they are added to the lane's own 64-bit
//                                 partials in memory every flush_tiles tiles, as many as 32 bits hold (never, unless the span is
//                                 large)
//   wide                          64-bit accumulators: four v_min_u32, two 32-bit adds of two minima (each below 2^31) and two
//                                 64-bit adds per pair and quad
// The launcher picks by span (memo_pairs_narrow_span() is the largest narrow one); the sums are exact either way.
// The accumulators leave once per workgroup: every lane's total (with what it has flushed) is summed over the position slots of its
// unit with wave shuffles, and slot 0 stores it to the partials, uint64 [grid.x][grid.y][256 lanes][64 cells].  pairs_reduce_kernel,
// one workgroup per unit, sums them over grid.x and the four waves and adds the sum to S[g][h] and S[h][g], each pair owned by one
// lane, launches ordered by the stream: no atomics.
//
// Conditions the code holds:
//   - no workgroup waits for another: no look-back, no flag in memory, no cooperative launch
//   - nothing is read outside [0, L) of a plane: a load that would cross L is made cell by cell for the cells before L.  The cells
//     [L, pitch) are never read
//   - vector loads, vector stores and plain C++ only; no inline assembly
//   - MEMO_EINVAL before any launch, the matrix as it was: d_cells not 16-byte aligned (or NULL where cells are read); pitch not a
//     multiple of 4 or below L; L < 0 or above 2^31; planes outside [0, 2048]; kmax outside [1, 2^31 - 1]; kmin outside [1, kmax];
//     a matrix that is NULL or not 8-byte aligned
//   - L == 0 or planes == 0 launches nothing and leaves the matrix as it was
//   - integer adds only, so the matrix depends neither on the slicing nor on the launch shape
//   - scratch: grid.x is cut so that the partials take at most 64 MiB, whatever planes and L are; DevPtr owns them; an allocation
//     that fails is MEMO_EHIP with the bytes asked for, and nothing stays allocated
#include <algorithm>
#include <vector>

#include "memo_common.h"

using namespace memo;

namespace memo {
thread_local int g_pairs_timed = 0;              // 1 = event pairs around the launches (memo_debug_pairs_times), each launch waited for
thread_local float g_pairs_ms[2] = {0.f, 0.f};  // ... of the last such call: the sweeps, the reduce launches
}

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64, kReduceThreads = 1024;
constexpr int kPer = 4;                        // uint32 cells in a 16-byte load: a quad
constexpr int kTile = 128, kQuads = kTile / kPer;
constexpr int kGroup = 8, kCells = kGroup * kGroup;  // genomes a group, pairs a unit
constexpr int kUnitsPerWg = 64;                // one unit a lane of a wave
constexpr int kMaxStaged = 128;                // genomes a launch stages at most (both chunks together): 64 KiB of LDS
constexpr int kMaxPlanes = 2048;
constexpr int kMaxGridX = 1024;                // runs of tiles at most
constexpr size_t kScratchCap = (size_t)64 << 20;
constexpr uint32_t kNarrowSpan = 0xFFFFFFFFu / kTile;  // the largest span with span x kTile < 2^32

struct PairArgs {
    const uint32_t *cells;  // [N][pitch]
    int64_t L, pitch, ntiles, tiles_per_wg, flush_tiles;
    int N;
    int ga0, na, gb0, nb;  // the staged genomes: [ga0, ga0 + na) and, for a rectangle (nb > 0), [gb0, gb0 + nb); na, nb multiples of 8
    int n8a, n8b;          // groups of eight in them
    int units;
    uint32_t kmax, below;  // below = kmin - 1
    uint64_t *partials;    // [gridDim.x][gridDim.y][kThreads][kCells]: every lane of the sweep its own 64
    uint64_t *sums;        // [N][N]
};

// the two groups of unit u (u < A.units)  (memo_cooc.hip's, duplicated: that file stays as it is)
__device__ __forceinline__ void unit_groups(const PairArgs &A, int u, int &a, int &b) {
    if (A.nb) {
        a = u % A.n8a;
        b = u / A.n8a;
        return;
    }
    b = (int)((sqrtf(8.f * (float)u + 1.f) - 1.f) * 0.5f);
    while ((b + 1) * (b + 2) / 2 <= u) ++b;
    while (b * (b + 1) / 2 > u) --b;
    a = u - b * (b + 1) / 2;
}

__device__ __forceinline__ uint32_t weight(uint32_t v, uint32_t kmax, uint32_t below) {
    const uint32_t m = min(v, kmax);
    return m > below ? m - below : 0u;
}

// the four cells at q of a plane; a cell at or past L is 0 and is not read
__device__ __forceinline__ uint4 load_cells(const uint32_t *__restrict__ v, int64_t q, int64_t L) {
    if (q + kPer <= L) return *reinterpret_cast<const uint4 *>(v + q);
    uint4 w;
    w.x = q < L ? v[q] : 0u;
    w.y = q + 1 < L ? v[q + 1] : 0u;
    w.z = q + 2 < L ? v[q + 2] : 0u;
    w.w = q + 3 < L ? v[q + 3] : 0u;
    return w;
}

// how many of a wave's 64 lanes a workgroup's `nu` units take, as a shift: the other lane bits number the position slots, so that a
// workgroup with few units still has work for every lane (at least 8 unit slots, at most 8 position slots: a tile has 32 quads for 4 waves)
__host__ __device__ __forceinline__ int unit_shift(int nu) {
    int sh = 3;
    while ((1 << sh) < nu) ++sh;
    return sh;
}

template <bool WIDE>
__global__ __launch_bounds__(kThreads) void pairs_kernel(const PairArgs A) {
    using acc_t = typename std::conditional<WIDE, uint64_t, uint32_t>::type;
    extern __shared__ __attribute__((aligned(16))) uint4 quads[];  // [staged genome][kQuads], rotated by the genome's group
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ubase = blockIdx.y * kUnitsPerWg, nu = min(A.units - ubase, kUnitsPerWg);
    const int ush = unit_shift(nu), nps = 64 >> ush;  // position slots a wave
    const int u = ubase + (lane & ((1 << ush) - 1)), pslot = lane >> ush;
    const bool active = u < A.units;
    int a = 0, b = 0;
    if (active) unit_groups(A, u, a, b);
    const int sb = (A.nb ? A.n8a : 0) + b;  // group b's number among the staged groups
    int staged = A.na + A.nb;
    if (!A.nb) {  // a triangle: no unit of this workgroup reads past the group of its last unit's b
        int la, lb;
        unit_groups(A, ubase + nu - 1, la, lb);
        staged = kGroup * (lb + 1);
    }
    acc_t acc[kCells] = {};
    bool first = true;
    // the lane's accumulators into its own partials: stored the first time, added to after (nobody else touches them)
    uint2 *mine = reinterpret_cast<uint2 *>(A.partials + (((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * kThreads + threadIdx.x) * kCells);
    auto flush = [&]() {
        if (!active) return;
#pragma unroll
        for (int c = 0; c < kCells; ++c) {  // (one base, constant offsets; in 32-bit halves: a 32-bit accumulator widened here is kept as a pair all along)
            const uint2 old = first ? make_uint2(0u, 0u) : mine[c];
            const uint32_t lo = old.x + (uint32_t)acc[c];
            mine[c] = make_uint2(lo, old.y + (uint32_t)((uint64_t)acc[c] >> 32) + (lo < old.x ? 1u : 0u));
            acc[c] = 0;
            if ((c & 7) == 7) __builtin_amdgcn_sched_barrier(0);  // (or the 64 loads are issued together, into 128 registers)
        }
        first = false;
    };
    // ... and at the end the lane's total, summed over the position slots of its unit with wave shuffles (every lane comes here: one
    // without a unit holds zeros), stored by slot 0: the reduce kernel reads one lane a unit and wave
    auto finish = [&]() {
#pragma unroll
        for (int c = 0; c < kCells; ++c) {
            const uint2 old = first ? make_uint2(0u, 0u) : mine[c];  // (in halves, as above)
            const uint32_t lo = old.x + (uint32_t)acc[c], hi = old.y + (uint32_t)((uint64_t)acc[c] >> 32) + (lo < old.x ? 1u : 0u);
            unsigned long long v = ((unsigned long long)hi << 32) | lo;
            for (int step = 1 << ush; step < 64; step <<= 1) v += __shfl_xor(v, step);
            if (active && pslot == 0) mine[c] = make_uint2((uint32_t)v, (uint32_t)(v >> 32));
        }
    };
    const int64_t t0 = (int64_t)blockIdx.x * A.tiles_per_wg, t1 = min(t0 + A.tiles_per_wg, A.ntiles);
    int64_t since = 0;  // tiles in the 32-bit accumulators
    for (int64_t t = t0; t < t1; ++t) {
        for (int item = threadIdx.x; item < staged * kQuads; item += kThreads) {
            const int s = item / kQuads, Q = item % kQuads;
            const int g = s < A.na ? A.ga0 + s : A.gb0 + s - A.na;
            const int64_t q = t * kTile + kPer * Q;
            uint4 w = make_uint4(0u, 0u, 0u, 0u);  // (a cell of 0 is a weight of 0)
            if (g < A.N && q < A.L) w = load_cells(A.cells + (int64_t)g * A.pitch, q, A.L);
            quads[s * kQuads + ((Q + (s >> 3)) & (kQuads - 1))] =
                make_uint4(weight(w.x, A.kmax, A.below), weight(w.y, A.kmax, A.below), weight(w.z, A.kmax, A.below), weight(w.w, A.kmax, A.below));
        }
        __syncthreads();
        if (active) {
#pragma unroll 1  // (unrolled, the reads of all its quads are hoisted: 256 VGPRs and 49 AGPRs)
            for (int Q = wave * nps + pslot; Q < kQuads; Q += kWaves * nps) {
                const uint4 *pa = quads + (kGroup * a) * kQuads + ((Q + a) & (kQuads - 1));
                const uint4 *pb = quads + (kGroup * sb) * kQuads + ((Q + sb) & (kQuads - 1));
                uint4 va[kGroup];
#pragma unroll
                for (int i = 0; i < kGroup; ++i) va[i] = pa[i * kQuads];
                uint4 vb = pb[0];
#pragma unroll
                for (int j = 0; j < kGroup; ++j) {
                    const uint4 cur = vb;
                    if (j + 1 < kGroup) vb = pb[(j + 1) * kQuads];  // (the next genome's read under this one's minima)
#pragma unroll
                    for (int i = 0; i < kGroup; ++i) {
                        if constexpr (WIDE) {  // two minima are below 2^32 together
                            acc[kGroup * i + j] += (uint64_t)(min(va[i].x, cur.x) + min(va[i].y, cur.y));
                            acc[kGroup * i + j] += (uint64_t)(min(va[i].z, cur.z) + min(va[i].w, cur.w));
                        } else {
                            acc[kGroup * i + j] += min(va[i].x, cur.x) + min(va[i].y, cur.y) + min(va[i].z, cur.z) + min(va[i].w, cur.w);
                        }
                    }
                }
            }
        }
        __syncthreads();
        if constexpr (!WIDE) {
            if (++since == A.flush_tiles && t + 1 < t1) {
                flush();
                since = 0;
            }
        }
    }
    finish();
}

// one workgroup per unit: lane (x = tid / 64, cell = tid % 64) sums its cell over every 16th of the sweep's waves that held the unit
// (one lane each: position slot 0), the 16 sums of a cell are added up through LDS, and the cell's owner adds the total to the matrix
// and to its mirror
__global__ __launch_bounds__(kReduceThreads) void pairs_reduce_kernel(const PairArgs A, int gx, int gy) {
    __shared__ uint64_t part[kReduceThreads];
    const int u = blockIdx.x, cell = threadIdx.x & (kCells - 1);
    const int y = u / kUnitsPerWg, slot = u % kUnitsPerWg;
    uint64_t sum = 0;
#pragma unroll 4
    for (int e = threadIdx.x / kCells; e < gx * kWaves; e += kReduceThreads / kCells)
        sum += A.partials[((((int64_t)(e / kWaves)) * gy + y) * kThreads + (e % kWaves) * 64 + slot) * kCells + cell];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x >= kCells) return;
    for (int x = 1; x < kReduceThreads / kCells; ++x) sum += part[kCells * x + cell];
    int a, b;
    unit_groups(A, u, a, b);
    const int g = A.ga0 + kGroup * a + cell / kGroup, h = (A.nb ? A.gb0 : A.ga0) + kGroup * b + cell % kGroup;
    if (!sum || g >= A.N || h >= A.N || g > h) return;
    A.sums[(int64_t)g * A.N + h] += sum;
    if (g != h) A.sums[(int64_t)h * A.N + g] += sum;
}

struct Launch {
    PairArgs A;
    int gx, gy;
    size_t lds_bytes() const { return (size_t)(A.na + A.nb) * kQuads * sizeof(uint4); }
    size_t scratch_bytes() const { return (size_t)gx * gy * kThreads * kCells * sizeof(uint64_t); }
};

// the launch of chunk pair (ca, cb) of the genomes, chunks of cg genomes
Launch plan(const uint32_t *d_cells, int64_t L, int64_t pitch, int N, uint32_t kmin, uint32_t kmax, int cg, int ca, int cb, uint64_t *d_sums) {
    PairArgs A = {};
    A.cells = d_cells;
    A.L = L;
    A.pitch = pitch;
    A.ntiles = (L + kTile - 1) / kTile;
    A.N = N;
    A.kmax = kmax;
    A.below = kmin - 1;
    A.sums = d_sums;
    auto groups = [&](int g0) { return (std::min(N - g0, cg) + kGroup - 1) / kGroup; };
    A.ga0 = ca * cg;
    A.n8a = groups(A.ga0);
    A.na = kGroup * A.n8a;
    if (cb != ca) {
        A.gb0 = cb * cg;
        A.n8b = groups(A.gb0);
        A.nb = kGroup * A.n8b;
    }
    A.units = A.nb ? A.n8a * A.n8b : A.n8a * (A.n8a + 1) / 2;
    Launch l = {};
    l.gy = (A.units + kUnitsPerWg - 1) / kUnitsPerWg;
    const int64_t by_scratch = (int64_t)(kScratchCap / ((size_t)l.gy * kThreads * kCells * sizeof(uint64_t)));
    const int64_t most = std::max<int64_t>(1, std::min<int64_t>({kMaxGridX, A.ntiles, by_scratch}));
    A.tiles_per_wg = (A.ntiles + most - 1) / most;
    l.gx = (int)((A.ntiles + A.tiles_per_wg - 1) / A.tiles_per_wg);
    // the tiles a 32-bit accumulator holds: a lane adds at most span a position (the wide form never asks)
    const uint64_t span = (uint64_t)kmax - kmin + 1;
    A.flush_tiles = std::max<int64_t>(1, (int64_t)(0xFFFFFFFFull / (span * kTile)));
    l.A = A;
    return l;
}

}  // namespace

extern "C" {

int32_t memo_pairs_tile(void) { return kTile; }
int32_t memo_pairs_chunk(void) { return kMaxStaged; }
uint32_t memo_pairs_narrow_span(void) { return kNarrowSpan; }

int memo_pairs_dev(const uint32_t *d_cells, int64_t L, int64_t pitch, int32_t planes, uint32_t kmin, uint32_t kmax, uint64_t *d_sums,
                   int32_t device, void *stream) {
    if (planes < 0 || planes > kMaxPlanes) return fail(MEMO_EINVAL, "planes must be in [0, %d] (planes = %d)", kMaxPlanes, planes);
    if (L < 0 || L > ((int64_t)1 << 31)) return fail(MEMO_EINVAL, "L = %lld: a plane holds at most 2^31 cells", (long long)L);
    if (pitch < L || (pitch & 3)) return fail(MEMO_EINVAL, "pitch %lld must be a multiple of 4 and at least L = %lld", (long long)pitch, (long long)L);
    if (kmax < 1 || kmax > 0x7fffffffu) return fail(MEMO_EINVAL, "kmax %u must be in [1, 2^31 - 1]", kmax);
    if (kmin < 1 || kmin > kmax) return fail(MEMO_EINVAL, "kmin %u must be in [1, kmax = %u]", kmin, kmax);
    if (reinterpret_cast<uintptr_t>(d_cells) & 15) return fail(MEMO_EINVAL, "d_cells must be 16-byte aligned");
    if (L && planes && !d_cells) return fail(MEMO_EINVAL, "d_cells is NULL");
    if (!d_sums || (reinterpret_cast<uintptr_t>(d_sums) & 7)) return fail(MEMO_EINVAL, "d_sums is NULL or not 8-byte aligned");
    if (!L || !planes) return MEMO_OK;

    const int cg = planes <= kMaxStaged ? kMaxStaged : kMaxStaged / 2, chunks = (planes + cg - 1) / cg;
    std::vector<Launch> launches;
    size_t scratch_bytes = 0;
    for (int ca = 0; ca < chunks; ++ca)
        for (int cb = ca; cb < chunks; ++cb) {
            launches.push_back(plan(d_cells, L, pitch, planes, kmin, kmax, cg, ca, cb, d_sums));
            scratch_bytes = std::max(scratch_bytes, launches.back().scratch_bytes());
        }
    const bool wide = kmax - kmin + 1 > kNarrowSpan;

    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DevPtr<uint64_t> scratch;  // one buffer, the launches take turns with it in stream order
    if (hipError_t err = scratch.alloc(scratch_bytes / sizeof(uint64_t)); err != hipSuccess)
        return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the partial sums of %d genomes: %s", scratch_bytes, planes, hipGetErrorString(err));
    Laps laps(st, g_pairs_timed, g_pairs_ms);  // (the launches add up)
    if (g_pairs_timed) g_pairs_ms[0] = g_pairs_ms[1] = 0.f;
    if (int rc = laps.start()) return rc;
    for (Launch &l : launches) {
        l.A.partials = scratch;
        const dim3 grid((unsigned)l.gx, (unsigned)l.gy);
        if (wide) hipLaunchKernelGGL(pairs_kernel<true>, grid, dim3(kThreads), l.lds_bytes(), st, l.A);
        else hipLaunchKernelGGL(pairs_kernel<false>, grid, dim3(kThreads), l.lds_bytes(), st, l.A);
        HIP_TRY(hipGetLastError());
        if (int rc = laps.add(0)) return rc;
        hipLaunchKernelGGL(pairs_reduce_kernel, dim3((unsigned)l.A.units), dim3(kReduceThreads), 0, st, l.A, l.gx, l.gy);
        HIP_TRY(hipGetLastError());
        if (int rc = laps.add(1)) return rc;
    }
    HIP_TRY(hipStreamSynchronize(st));
    return MEMO_OK;
}

}  // extern "C"
