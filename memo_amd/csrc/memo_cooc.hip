// memo_cooc.hip -- `memo matrix`: the co-occurrence matrix of a membership result that is still in HBM,
//     C[g][h] += #{ p in [0, L) : bit g and bit h of row p are set }          0 <= g, h < num_docs, uint64
// so that num_docs x num_docs integers and not L rows leave the device.  No counterpart in the reference.  The first product here
// that is a reduction over positions and not a map: it shares nothing with memo_runs.hip or the binning kernel but the conventions.
//
// Pair space.  Genomes come in groups of four; a UNIT is a pair of groups (a, b), a 4 x 4 block of genome pairs, 16 32-bit
// accumulators in one lane.  Only units with a <= b exist (the upper triangle; the lower one is mirrored when the counts leave), they
// are numbered b (b + 1) / 2 + a, and a workgroup of 256 lanes owns 256 x KU consecutive units (KU = 1 up to 256 units, else 2:
// 16 or 32 accumulators a lane, whatever num_docs is): grid.y walks the pair space, grid.x the positions.
// Genome words are taken at most 16 at a time (512 genomes): above that the words are cut into chunks of 8, and one launch per pair
// of chunks (ca <= cb) stages both chunks; ca < cb is a full rectangle of units, not a triangle.  Right for every num_docs >= 1,
// made to be fast up to 512.
//
// One tile = 512 positions = 16 position words.  Per tile a workgroup
//   1. stages: one lane per (staged genome word s, position word P) loads the 32 row words of its 32 x 32 block, masks the bits at
//      or above num_docs, transposes the block in registers (transpose32: memo_planes.h, shared with memo_collect.hip) and writes the 32 plane
//      words -- plane[P][genome] holds 32 positions of one genome -- to LDS with eight 16-byte stores.  A block is 36 words apart
//      from the next and a position word's row 36 x staged + 4: the 16-byte stores of the lanes then fall on all banks alike.
//      A triangle workgroup stages only the words up to that of its largest b.
//   2. accumulates: per position word and unit two 16-byte LDS reads (the four planes of a, of b) and 16 x (v_and_b32,
//      v_bcnt_u32_b32 with its accumulate operand).
// The accumulators live across all the tiles a workgroup takes (a run of consecutive tiles) and leave once:
//   partials (the product's way)  16 uint32 per unit and workgroup into a scratch buffer [grid.x][units][16]; cooc_reduce_kernel sums
//                                 them over grid.x in 64 bits and adds the sum to counts[g][h] and counts[h][g], each pair owned by
//                                 one lane, launches ordered by the stream: no atomics at all
//   atomics (A/B: memo_debug_cooc_flush of the AB library)  one 64-bit atomicAdd per pair, mirror and workgroup
// Integer addition is exact in any order: both give the same matrix (DESIGN.md 10.4 has both times).
//
// Conditions the code holds:
//   - no workgroup waits for another: no look-back, no flag in memory, no cooperative launch
//   - nothing is read outside d_bits[0 .. L * W): every load is of one row word, and a block that crosses L loads row by row, the
//     rows before L only (a row at or past L counts as zeros)
//   - a d_bits that is not 16-byte aligned is MEMO_EINVAL before any launch; L == 0 launches nothing and leaves d_counts as it was
//   - bits at or above num_docs never reach a count: they are masked as the words are loaded, the encoding is not trusted
//   - L and positions are int64; the matrix is 64-bit
//   - the 32-bit accumulators cannot wrap: an accumulator gains at most 1 per position, a workgroup takes tiles_per_wg tiles of 512
//     positions, and the launcher refuses (MEMO_EINVAL) a result that would make tiles_per_wg exceed 2^22, i.e. 2^31 positions
//   - scratch: grid.x is cut so that the partials take at most 64 MiB, whatever num_docs and L are; DevPtr owns them until the
//     call has succeeded; an allocation that fails is MEMO_EHIP with the bytes asked for, and nothing stays allocated
// Also here: memo_query_membership_slice_dev, the sweep of one slice of a window as part of that window -- what lets a caller
// accumulate a window slice by slice (memo_amd/matrix.py: region_matrix) and get the window's matrix.
#include <algorithm>

#include "memo_planes.h"

using namespace memo;

namespace memo {
thread_local int g_cooc_flush = 0;  // 0 = partials + reduce, 1 = 64-bit atomics (memo_debug_cooc_flush)
thread_local int g_cooc_timed = 0;  // 1 = event pairs around the launches (memo_debug_cooc_times), each launch waited for
thread_local float g_cooc_ms[2] = {0.f, 0.f};  // ... of the last such call: the sweeps, the reduce launches
}

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 512, kPW = kTile / 32;  // positions per tile, its position words
constexpr int kBlockPitch = kPlaneBlockPitch;  // LDS words from one staged genome word to the next
constexpr int kMaxStaged = 16;                // genome words a launch stages at most (both chunks together)
constexpr int kMaxGridX = 1024;               // workgroups along the positions at most
constexpr size_t kScratchCap = (size_t)64 << 20;
constexpr int64_t kMaxTilesPerWg = (int64_t)1 << 22;  // x 512 positions = 2^31: what keeps 32-bit accumulators exact

struct CoocArgs {
    const uint32_t *bits;
    int64_t L, ntiles, tiles_per_wg;
    int W, N;
    int wa0, nwa, wb0, nwb;  // the staged genome words: [wa0, wa0 + nwa) and, for a rectangle (nwb > 0), [wb0, wb0 + nwb)
    int n4a, n4b;            // groups of four genomes in them
    int units, pitch;        // pitch: LDS words per position word
    uint32_t *partials;      // nullptr: atomics
    uint64_t *counts;
};

// the two groups of unit u (u < A.units)
__device__ __forceinline__ void unit_groups(const CoocArgs &A, int u, int &a, int &b) {
    if (A.nwb) {
        a = u % A.n4a;
        b = u / A.n4a;
        return;
    }
    b = (int)((sqrtf(8.f * (float)u + 1.f) - 1.f) * 0.5f);
    while ((b + 1) * (b + 2) / 2 <= u) ++b;
    while (b * (b + 1) / 2 > u) --b;
    a = u - b * (b + 1) / 2;
}

__device__ __forceinline__ int first_genome_a(const CoocArgs &A, int a) { return 32 * A.wa0 + 4 * a; }
__device__ __forceinline__ int first_genome_b(const CoocArgs &A, int b) { return 32 * (A.nwb ? A.wb0 : A.wa0) + 4 * b; }
// LDS words from a position word's row to the four planes of group g4 of the staged words from `staged_base` on
__device__ __forceinline__ int plane_offset(int staged_base, int g4) { return kBlockPitch * (staged_base + (g4 >> 3)) + 4 * (g4 & 7); }

// whether cell (i, j) of a unit is a pair of the upper triangle, diagonal included, with both genomes below N
__device__ __forceinline__ bool cell_counts(const CoocArgs &A, int g, int h) { return g < A.N && h < A.N && g <= h; }

template <int KU>
__global__ __launch_bounds__(kThreads) void cooc_kernel(const CoocArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint32_t planes[];
    const int lane = threadIdx.x & 63;
    // which of the workgroup's four runs of 64 units a wave takes turns with the workgroup: the last run of a pair space is
    // seldom full, and the same wave of every workgroup should not be the one that has less to do
    const int vwave = ((threadIdx.x >> 6) + blockIdx.x) & 3, vt = vwave * 64 + lane;
    const int ubase = blockIdx.y * (kThreads * KU);
    int offa[KU], offb[KU];
#pragma unroll
    for (int q = 0; q < KU; ++q) {
        const int u = ubase + q * kThreads + vt;
        int a = 0, b = 0;
        if (u < A.units) unit_groups(A, u, a, b);
        offa[q] = plane_offset(0, a);
        offb[q] = plane_offset(A.nwb ? A.nwa : 0, b);
    }
    int staged = A.nwa + A.nwb;
    if (!A.nwb) {  // a triangle: no unit of this workgroup reads past the word of its last unit's b
        int a, b;
        unit_groups(A, min(A.units, ubase + kThreads * KU) - 1, a, b);
        staged = (b >> 3) + 1;
    }
    uint32_t acc[KU][16] = {};
    const int64_t t0 = (int64_t)blockIdx.x * A.tiles_per_wg, t1 = min(t0 + A.tiles_per_wg, A.ntiles);
    for (int64_t t = t0; t < t1; ++t) {
        // (at most one block a lane: staged <= 16.  Few genome words are one wave's work or less -- 64 blocks at W = 4 --: the wave
        // that does it changes with the tile, so that no SIMD of the CU stages for all the tiles)
        for (int blk = (threadIdx.x + 64 * (int)(t & 3)) & (kThreads - 1); blk < staged * kPW; blk += kThreads) {
            const int s = blk % staged, P = blk / staged;
            const int w = s < A.nwa ? A.wa0 + s : A.wb0 + s - A.nwa;
            const int64_t r0 = t * kTile + 32 * P;
            const uint32_t *src = A.bits + r0 * A.W + w;
            uint32_t m[32];
            if (r0 + 32 <= A.L) {
#pragma unroll
                for (int i = 0; i < 32; ++i) m[i] = src[(int64_t)i * A.W];
            } else {
#pragma unroll
                for (int i = 0; i < 32; ++i) m[i] = r0 + i < A.L ? src[(int64_t)i * A.W] : 0u;
            }
            const uint32_t below_n = (w == A.W - 1 && (A.N & 31)) ? (1u << (A.N & 31)) - 1u : 0xFFFFFFFFu;
#pragma unroll
            for (int i = 0; i < 32; ++i) m[i] &= below_n;
            transpose32(m);  // m[j]: genome 32 w + j, bit i: position r0 + i
            uint4 *dst = reinterpret_cast<uint4 *>(planes + P * A.pitch + kBlockPitch * s);
#pragma unroll
            for (int q = 0; q < 8; ++q) dst[q] = make_uint4(m[4 * q], m[4 * q + 1], m[4 * q + 2], m[4 * q + 3]);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < KU; ++q) {
            if (ubase + q * kThreads + vwave * 64 >= A.units) continue;  // (the whole wave: no unit there)
#pragma unroll 4
            for (int P = 0; P < kPW; ++P) {
                const uint32_t *row = planes + P * A.pitch;
                const uint4 a4 = *reinterpret_cast<const uint4 *>(row + offa[q]), b4 = *reinterpret_cast<const uint4 *>(row + offb[q]);
                const uint32_t a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[q][4 * i + j] += (uint32_t)__popc(a[i] & b[j]);
            }
        }
        __syncthreads();
    }
    if (A.partials) {
        const int64_t slots = (int64_t)gridDim.y * (kThreads * KU);
#pragma unroll
        for (int q = 0; q < KU; ++q) {
            uint4 *dst = reinterpret_cast<uint4 *>(A.partials + ((int64_t)blockIdx.x * slots + ubase + q * kThreads + vt) * 16);
#pragma unroll
            for (int i = 0; i < 4; ++i) dst[i] = make_uint4(acc[q][4 * i], acc[q][4 * i + 1], acc[q][4 * i + 2], acc[q][4 * i + 3]);
        }
        return;
    }
#pragma unroll
    for (int q = 0; q < KU; ++q) {
        const int u = ubase + q * kThreads + vt;
        if (u >= A.units) continue;
        int a, b;
        unit_groups(A, u, a, b);
        const int g0 = first_genome_a(A, a), h0 = first_genome_b(A, b);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int g = g0 + i, h = h0 + j;
                const unsigned long long v = acc[q][4 * i + j];
                if (!v || !cell_counts(A, g, h)) continue;
                atomicAdd(reinterpret_cast<unsigned long long *>(A.counts) + (int64_t)g * A.N + h, v);
                if (g != h) atomicAdd(reinterpret_cast<unsigned long long *>(A.counts) + (int64_t)h * A.N + g, v);
            }
    }
}

// one workgroup per unit: lane (x lane = tid / 16, cell = tid % 16) sums its cell over every 16th workgroup of the sweep's grid.x,
// the 16 sums of a cell are added up through LDS, and the cell's owner adds the total to the matrix and to its mirror
__global__ __launch_bounds__(kThreads) void cooc_reduce_kernel(const CoocArgs A, int gx, int64_t slots) {
    __shared__ uint64_t part[kThreads];
    const int u = blockIdx.x, cell = threadIdx.x & 15;
    uint64_t sum = 0;
    for (int x = threadIdx.x >> 4; x < gx; x += kThreads / 16) sum += A.partials[((int64_t)x * slots + u) * 16 + cell];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x >= 16) return;
    for (int x = 1; x < kThreads / 16; ++x) sum += part[16 * x + cell];
    int a, b;
    unit_groups(A, u, a, b);
    const int g = first_genome_a(A, a) + (cell >> 2), h = first_genome_b(A, b) + (cell & 3);
    if (!sum || !cell_counts(A, g, h)) return;
    A.counts[(int64_t)g * A.N + h] += sum;
    if (g != h) A.counts[(int64_t)h * A.N + g] += sum;
}

struct Launch {
    CoocArgs A;
    int ku, gx, gy;
    int64_t slots;
    size_t scratch_bytes() const { return (size_t)gx * (size_t)slots * 16 * sizeof(uint32_t); }
};

// the launch of chunk pair (ca, cb) of the genome words, chunks of cw words
int plan(const uint32_t *d_bits, int64_t L, int N, int cw, int ca, int cb, bool partials, uint64_t *d_counts, Launch *out) {
    const int W = (N + 31) / 32;
    CoocArgs A = {};
    A.bits = d_bits;
    A.L = L;
    A.ntiles = (L + kTile - 1) / kTile;
    A.W = W;
    A.N = N;
    A.counts = d_counts;
    auto groups = [&](int w0, int nw) { return (std::min(N - 32 * w0, 32 * nw) + 3) / 4; };
    A.wa0 = ca * cw;
    A.nwa = std::min(cw, W - A.wa0);
    A.n4a = groups(A.wa0, A.nwa);
    if (cb != ca) {
        A.wb0 = cb * cw;
        A.nwb = std::min(cw, W - A.wb0);
        A.n4b = groups(A.wb0, A.nwb);
    }
    A.units = A.nwb ? A.n4a * A.n4b : A.n4a * (A.n4a + 1) / 2;
    A.pitch = kBlockPitch * (A.nwa + A.nwb) + 4;
    Launch l = {};
    l.ku = A.units <= kThreads ? 1 : 2;
    l.gy = (A.units + kThreads * l.ku - 1) / (kThreads * l.ku);
    l.slots = (int64_t)l.gy * kThreads * l.ku;
    int64_t cap = std::min<int64_t>(kMaxGridX, A.ntiles);
    if (partials) cap = std::min<int64_t>(cap, std::max<int64_t>(1, (int64_t)(kScratchCap / ((size_t)l.slots * 64))));
    A.tiles_per_wg = (A.ntiles + cap - 1) / cap;
    if (A.tiles_per_wg > kMaxTilesPerWg) return fail(MEMO_EINVAL, "a result of %lld positions is too long", (long long)L);
    l.gx = (int)((A.ntiles + A.tiles_per_wg - 1) / A.tiles_per_wg);
    l.A = A;
    *out = l;
    return MEMO_OK;
}

template <int KU>
void launch_sweep(const Launch &l, hipStream_t st) {
    hipLaunchKernelGGL(cooc_kernel<KU>, dim3((unsigned)l.gx, (unsigned)l.gy), dim3(kThreads), (size_t)kPW * l.A.pitch * sizeof(uint32_t), st,
                       l.A);
}

}  // namespace

extern "C" {

int32_t memo_cooccurrence_tile(int32_t words) { return kTile; }

int memo_cooccurrence_dev(const uint32_t *d_bits, int64_t L, int32_t num_docs, uint64_t *d_counts, int32_t device, void *stream) {
    if (num_docs < 1) return fail(MEMO_EINVAL, "num_docs must be at least 1");
    if (L < 0 || (L && !d_bits)) return fail(MEMO_EINVAL, "bad membership result (L = %lld)", (long long)L);
    if (!d_counts || (reinterpret_cast<uintptr_t>(d_counts) & 7)) return fail(MEMO_EINVAL, "d_counts is NULL or not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_bits) & 15) return fail(MEMO_EINVAL, "d_bits must be 16-byte aligned");
    if (!L) return MEMO_OK;
    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool partials = g_cooc_flush == 0;
    const int W = (num_docs + 31) / 32, cw = W <= kMaxStaged ? W : kMaxStaged / 2, chunks = (W + cw - 1) / cw;
    std::vector<Launch> launches;
    size_t scratch_bytes = 0;
    for (int ca = 0; ca < chunks; ++ca)
        for (int cb = ca; cb < chunks; ++cb) {
            Launch l;
            if (int rc = plan(d_bits, L, num_docs, cw, ca, cb, partials, d_counts, &l)) return rc;
            if (partials && l.scratch_bytes() > scratch_bytes) scratch_bytes = l.scratch_bytes();
            launches.push_back(l);
        }
    DevPtr<uint32_t> scratch;  // one buffer, the launches take turns with it in stream order
    if (partials)
        if (hipError_t err = scratch.alloc(scratch_bytes / sizeof(uint32_t)); err != hipSuccess)
            return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the partial counts of %d genomes: %s", scratch_bytes, num_docs, hipGetErrorString(err));
    Laps laps(st, g_cooc_timed, g_cooc_ms);  // (the launches add up)
    if (g_cooc_timed) g_cooc_ms[0] = g_cooc_ms[1] = 0.f;
    if (int rc = laps.start()) return rc;
    for (Launch &l : launches) {
        l.A.partials = scratch;
        if (l.ku == 1) launch_sweep<1>(l, st);
        else launch_sweep<2>(l, st);
        HIP_TRY(hipGetLastError());
        if (int rc = laps.add(0)) return rc;
        if (partials) {
            hipLaunchKernelGGL(cooc_reduce_kernel, dim3((unsigned)l.A.units), dim3(kThreads), 0, st, l.A, l.gx, l.slots);
            HIP_TRY(hipGetLastError());
        }
        if (int rc = laps.add(1)) return rc;
    }
    HIP_TRY(hipStreamSynchronize(st));
    return MEMO_OK;
}

// A slice of a window, swept as part of it.  A row with end < start reaches any distance left of its start, so the reference's
// filter (memo_query.py:25-27) lets it through by the WHOLE window: swept alone, a slice would see other rows than the window does
// (memo_common.h: whole_set; memo_multi.hip sweeps its sub-windows the same way).
int memo_query_membership_slice_dev(memo_index_t *ix, int64_t whole_qs, int64_t whole_qe, int64_t qs, int64_t qe, int32_t k,
                                    int32_t num_docs, uint32_t *d_out, void *stream) {
    if (!ix) return fail(MEMO_EINVAL, "index is NULL");
    if (whole_qe < whole_qs) return fail(MEMO_EINVAL, "ValueError: negative dimensions are not allowed (window end < start)");
    if (qs < whole_qs || qe > whole_qe) return fail(MEMO_EINVAL, "the slice [%lld, %lld) leaves its window [%lld, %lld)", (long long)qs,
                                                    (long long)qe, (long long)whole_qs, (long long)whole_qe);
    struct WholeWindow {
        memo_index_t *ix;
        WholeWindow(memo_index_t *i, int64_t s, int64_t e) : ix(i) { ix->whole_qs = s, ix->whole_qe = e, ix->whole_set = 1; }
        ~WholeWindow() { ix->whole_set = 0; }
    } whole(ix, whole_qs, whole_qe);
    return memo_query_membership_dev(ix, qs, qe, k, num_docs, d_out, stream);
}

}  // extern "C"
