// memo_collect.hip -- `memo collect`: the collector's curves of a membership result that is still in HBM.  For every order q (a row of
// `steps` genome ids) and every step j
//     core   [q][j] += #{ p in [0, L) : bit orders[q][i] of row p is set for every i <= j }
//     covered[q][j] += #{ p in [0, L) : bit orders[q][i] of row p is set for some  i <= j }                 uint64 [orders][steps]
// so that orders x steps integers and not L rows leave the device.  No counterpart in the reference.  The second reduction over
// positions after memo_cooc.hip: the same per-genome bit planes (memo_planes.h), but a dependent chain per order, not independent pairs.
//
// One tile = PW position words = 32 PW positions; PW = 16 up to 16 genome words (512 positions a tile), 8 up to 32, 4 up to 64: more
// genome words shrink the tile and not the genomes staged, because the chain over an order cannot be cut the way pairs can.  A
// workgroup of 256 lanes takes a run of consecutive tiles (grid.x) and a block of `ob` orders (grid.y); lane = (order tid / PW,
// position word tid % PW), ob <= 256 / PW, and fewer where the orders' LDS would pass kLdsBudget (lanes past ob idle: right for every
// steps <= num_docs <= 2048, made to be fast up to about 128 steps).  LDS: the planes as memo_cooc.hip lays them out, two uint32
// accumulators per (order, step), the block's orders as uint16 (each genome as the place of its plane word in a row); steps are
// padded to a multiple of 8 with the order's first genome (and and or are idempotent; the padding's accumulators never leave).
// Per tile a workgroup
//   1. stages the planes (stage_plane_block: one load per row word, rows at or past L as zeros, bits at or above num_docs masked,
//      transpose32, 16-byte stores at the 36-word pitch), at most one block a lane;
//   2. walks: each lane its order, eight steps at a time -- one 16-byte read of eight genomes' places, eight plane words, and per step
//      a &= x, o |= x, popc(a) | popc(o) << 16 summed over the PW lanes of the row with log2(PW) DPP adds (each count is at most 32, a
//      sum at most 512: the packing is exact); lane 0 of the row adds the two halves to the step's accumulators, a plain
//      read-modify-write by the only lane that owns them, no LDS atomic.
// The accumulators live across all the tiles a workgroup takes and leave once as partials uint32 [grid.x][orders][steps][2];
// collect_reduce_kernel sums them over grid.x in 64 bits and adds the sums to core and covered: every cell has one owner and the
// stream orders the launches, so there are no global atomics.  Orders are taken in batches where the partials of all would pass the
// scratch cap.
//
// Conditions the code holds:
//   - no workgroup waits for another: no look-back, no flag in memory, no cooperative launch
//   - nothing is read outside d_bits[0 .. L * W): every load is of one row word, of the rows before L only
//   - a d_bits that is not 16-byte aligned is MEMO_EINVAL before any launch
//   - `orders` is a HOST pointer: the library validates it (an entry >= num_docs, steps outside [1, num_docs], num_orders outside
//     [0, 65535], num_docs > 65535 are MEMO_EINVAL before any launch; so is num_docs > kMaxDocs = 2048) and uploads it itself
//   - L == 0 or num_orders == 0 launches nothing and leaves the outputs as they were
//   - bits at or above num_docs never reach a count: they are masked as the words are loaded, the encoding is not trusted
//   - L and positions are int64; the curves are 64-bit
//   - the 32-bit accumulators cannot wrap: one gains at most 512 per tile, and the launcher refuses (MEMO_EINVAL) what would give a
//     workgroup more than 2^22 tiles
//   - scratch: grid.x and the batch of orders are cut so that the partials take at most 64 MiB, whatever the arguments are; DevPtr
//     owns them and the uploaded orders behind them (one allocation); an allocation that fails is MEMO_EHIP with the bytes asked for, and nothing stays allocated
//   - vector stores and plain C++ only
#include <algorithm>
#include <map>

#include "memo_planes.h"

using namespace memo;

namespace memo {
thread_local int g_collect_timed = 0;  // 1 = event pairs around the launches (memo_debug_collect_times), each launch waited for
thread_local float g_collect_ms[2] = {0.f, 0.f};  // ... of the last such call: the sweeps, the reduce launches
}

namespace {

constexpr int kThreads = 256;
constexpr int kMaxDocs = 2048;                // 64 genome words: the planes of a 4-word tile are 36 KiB
constexpr int kMaxGridX = 1024;               // workgroups along the positions at most
constexpr int kStepChunk = 8;                 // steps a lane takes at a time
constexpr size_t kLdsBudget = (size_t)120 << 10;  // of the CU's 160 KiB: 16 orders of 511 steps beside the planes of 16 genome words
constexpr size_t kScratchCap = (size_t)64 << 20;
constexpr int64_t kMaxTilesPerWg = (int64_t)1 << 22;  // x 512 per tile at most = 2^31: what keeps 32-bit accumulators exact

struct CollectArgs {
    const uint32_t *bits;
    int64_t L, ntiles, tiles_per_wg;
    int W, N;
    int P, M, Mp;            // the orders of this launch, their steps, the steps rounded up to kStepChunk
    int ob;                  // orders a workgroup takes
    int pitch;               // LDS words per position word
    const uint16_t *orders;  // [P][M], on the device
    uint32_t *partials;      // [grid.x][P][M][2]
    uint64_t *core, *covered;  // [P][M]
};

inline int position_words(int W) { return W <= 16 ? 16 : W <= 32 ? 8 : 4; }

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_add(uint32_t v) {
    return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}

// the sum of v over the PW lanes of a row (aligned runs of PW lanes), in every one of them
template <int PW>
__device__ __forceinline__ uint32_t row_sum(uint32_t v) {
    v = dpp_add<0xB1>(v);                   // quad_perm [1, 0, 3, 2]: lane ^ 1
    v = dpp_add<0x4E>(v);                   // quad_perm [2, 3, 0, 1]: lane ^ 2
    if (PW >= 8) v = dpp_add<0x141>(v);     // row_half_mirror: lane i of eight takes 7 - i, the other quad's sum
    if (PW >= 16) v = dpp_add<0x140>(v);    // row_mirror: lane i of sixteen takes 15 - i, the other half's sum
    return v;
}

template <int PW>
__global__ __launch_bounds__(kThreads) void collect_kernel(const CollectArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint32_t planes[];
    uint2 *acc = reinterpret_cast<uint2 *>(planes + PW * A.pitch);       // [ob][Mp]: core, covered
    uint16_t *ord = reinterpret_cast<uint16_t *>(acc + A.ob * A.Mp);     // [ob][Mp]: below 36 x 64 words
    const int q0 = blockIdx.y * A.ob, nq = min(A.ob, A.P - q0);
    for (int i = threadIdx.x; i < nq * A.Mp; i += kThreads) {
        const int o = i / A.Mp, j = i % A.Mp;
        acc[i] = make_uint2(0u, 0u);
        const uint32_t g = A.orders[(int64_t)(q0 + o) * A.M + (j < A.M ? j : 0)];
        ord[i] = (uint16_t)(kPlaneBlockPitch * (g >> 5) + (g & 31u));  // where genome g's plane word lies in a position word's row
    }
    const int o = threadIdx.x / PW, pword = threadIdx.x % PW;
    const uint32_t *row = planes + pword * A.pitch;
    const uint16_t *my_order = ord + o * A.Mp;
    uint2 *my_acc = acc + o * A.Mp;
    const int staged = A.W * PW;  // blocks a tile has: at most one a lane
    const int64_t t0 = (int64_t)blockIdx.x * A.tiles_per_wg, t1 = min(t0 + A.tiles_per_wg, A.ntiles);
    for (int64_t t = t0; t < t1; ++t) {
        // (few genome words are one wave's work or less: the wave that does it changes with the tile, as in cooc_kernel)
        for (int blk = (threadIdx.x + 64 * (int)(t & 3)) & (kThreads - 1); blk < staged; blk += kThreads) {
            const int w = blk % A.W, P = blk / A.W;
            stage_plane_block(A.bits, A.L, A.W, A.N, w, t * (32 * PW) + 32 * P, planes + P * A.pitch + kPlaneBlockPitch * w);
        }
        __syncthreads();  // (the first one also orders the fill of acc and ord above)
        if (o < nq) {     // (whole rows of PW lanes: the lanes a DPP add reads are active)
            uint32_t a = 0xFFFFFFFFu, r = 0u;
            for (int j0 = 0; j0 < A.Mp; j0 += kStepChunk) {
                const uint4 g8 = *reinterpret_cast<const uint4 *>(my_order + j0);
                const uint32_t at[kStepChunk] = {g8.x & 0xFFFFu, g8.x >> 16, g8.y & 0xFFFFu, g8.y >> 16,
                                                g8.z & 0xFFFFu, g8.z >> 16, g8.w & 0xFFFFu, g8.w >> 16};
                uint32_t x[kStepChunk], s[kStepChunk];
#pragma unroll
                for (int i = 0; i < kStepChunk; ++i) x[i] = row[at[i]];
#pragma unroll
                for (int i = 0; i < kStepChunk; ++i) {
                    a &= x[i];
                    r |= x[i];
                    s[i] = row_sum<PW>((uint32_t)__popc(a) | (uint32_t)__popc(r) << 16);
                }
                if (pword == 0) {
                    uint4 *cells = reinterpret_cast<uint4 *>(my_acc + j0);
#pragma unroll
                    for (int i = 0; i < kStepChunk / 2; ++i) {
                        uint4 v = cells[i];
                        v.x += s[2 * i] & 0xFFFFu;
                        v.y += s[2 * i] >> 16;
                        v.z += s[2 * i + 1] & 0xFFFFu;
                        v.w += s[2 * i + 1] >> 16;
                        cells[i] = v;
                    }
                }
            }
        }
        __syncthreads();
    }
    uint2 *out = reinterpret_cast<uint2 *>(A.partials) + ((int64_t)blockIdx.x * A.P + q0) * A.M;
    for (int i = threadIdx.x; i < nq * A.M; i += kThreads) out[i] = acc[(i / A.M) * A.Mp + i % A.M];
}

// one workgroup per 16 cells (order, step): lane (x lane = tid / 16, cell = tid % 16) sums its cell over every 16th workgroup of the
// sweep's grid.x, the 16 sums of a cell are added up through LDS, and the cell's owner adds the totals to the two curves
__global__ __launch_bounds__(kThreads) void collect_reduce_kernel(const CollectArgs A, int gx) {
    __shared__ uint64_t part[2][kThreads];
    const int64_t cells = (int64_t)A.P * A.M, cell = (int64_t)blockIdx.x * 16 + (threadIdx.x & 15);
    uint64_t core = 0, covered = 0;
    if (cell < cells)
        for (int x = threadIdx.x >> 4; x < gx; x += kThreads / 16) {
            const uint2 v = reinterpret_cast<const uint2 *>(A.partials)[(int64_t)x * cells + cell];
            core += v.x;
            covered += v.y;
        }
    part[0][threadIdx.x] = core;
    part[1][threadIdx.x] = covered;
    __syncthreads();
    if (threadIdx.x >= 16 || cell >= cells) return;
    for (int x = 1; x < kThreads / 16; ++x) core += part[0][16 * x + threadIdx.x], covered += part[1][16 * x + threadIdx.x];
    A.core[cell] += core;
    A.covered[cell] += covered;
}

template <int PW>
int launch_sweep(const CollectArgs &A, int gx, int gy, size_t lds, hipStream_t st) {
    if (lds > 64 * 1024) {  // opt in to large dynamic LDS once per (thread, device, size)
        thread_local std::map<int, size_t> granted;
        int dev = 0;
        HIP_TRY(hipGetDevice(&dev));
        size_t &have = granted[dev];
        if (have < lds) {
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(collect_kernel<PW>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            have = lds;
        }
    }
    hipLaunchKernelGGL(collect_kernel<PW>, dim3((unsigned)gx, (unsigned)gy), dim3(kThreads), lds, st, A);
    HIP_TRY(hipGetLastError());
    return MEMO_OK;
}

}  // namespace

extern "C" {

int32_t memo_collect_tile(int32_t words) { return 32 * position_words(words); }

int memo_collect_dev(const uint32_t *d_bits, int64_t L, int32_t num_docs, const uint16_t *orders_host, int32_t num_orders, int32_t steps,
                     uint64_t *d_core, uint64_t *d_covered, int32_t device, void *stream) {
    if (num_docs < 1 || num_docs > 65535) return fail(MEMO_EINVAL, "num_docs must be in [1, 65535]");
    if (num_docs > kMaxDocs) return fail(MEMO_EINVAL, "collector's curves are made for at most %d genomes (num_docs = %d)", kMaxDocs, num_docs);
    if (L < 0 || (L && !d_bits)) return fail(MEMO_EINVAL, "bad membership result (L = %lld)", (long long)L);
    if (num_orders < 0 || num_orders > 65535) return fail(MEMO_EINVAL, "num_orders must be in [0, 65535]");
    if (steps < 1 || steps > num_docs) return fail(MEMO_EINVAL, "steps must be in [1, num_docs] (steps = %d, num_docs = %d)", steps, num_docs);
    if (num_orders && !orders_host) return fail(MEMO_EINVAL, "orders is NULL");
    if (!d_core || !d_covered || ((reinterpret_cast<uintptr_t>(d_core) | reinterpret_cast<uintptr_t>(d_covered)) & 7))
        return fail(MEMO_EINVAL, "d_core or d_covered is NULL or not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_bits) & 15) return fail(MEMO_EINVAL, "d_bits must be 16-byte aligned");
    const int P = num_orders, M = steps, N = num_docs;
    for (int64_t i = 0; i < (int64_t)P * M; ++i)
        if (orders_host[i] >= N)
            return fail(MEMO_EINVAL, "order %lld, step %lld: genome %d of %d", (long long)(i / M), (long long)(i % M), (int)orders_host[i], N);
    if (!L || !P) return MEMO_OK;

    CollectArgs A = {};
    A.bits = d_bits;
    A.L = L;
    A.W = (N + 31) / 32;
    A.N = N;
    A.M = M;
    A.Mp = (M + kStepChunk - 1) / kStepChunk * kStepChunk;
    A.pitch = kPlaneBlockPitch * A.W + 4;
    A.core = d_core;
    A.covered = d_covered;
    const int pw = position_words(A.W);
    A.ntiles = (L + 32 * pw - 1) / (32 * pw);
    const size_t plane_bytes = (size_t)pw * A.pitch * sizeof(uint32_t), order_bytes = (size_t)A.Mp * (sizeof(uint2) + sizeof(uint16_t));
    A.ob = (int)std::min<size_t>(std::min(kThreads / pw, P), std::max<size_t>(1, (kLdsBudget - plane_bytes) / order_bytes));
    const size_t lds = plane_bytes + A.ob * order_bytes;
    // the partials of a launch: grid.x x its orders x steps x 8 bytes, at most kScratchCap.  grid.x gives way first, down to what lets
    // 256 orders (or all) go in one launch; then the orders go in batches
    const size_t step_bytes = (size_t)M * 2 * sizeof(uint32_t);
    const int64_t gx_cap = std::max<int64_t>(1, (int64_t)(kScratchCap / (step_bytes * std::min(P, 256))));
    const int64_t cap = std::min<int64_t>({(int64_t)kMaxGridX, A.ntiles, gx_cap});
    A.tiles_per_wg = (A.ntiles + cap - 1) / cap;
    if (A.tiles_per_wg > kMaxTilesPerWg) return fail(MEMO_EINVAL, "a result of %lld positions is too long", (long long)L);
    const int gx = (int)((A.ntiles + A.tiles_per_wg - 1) / A.tiles_per_wg);
    int batch = (int)std::min<int64_t>(P, (int64_t)(kScratchCap / (step_bytes * gx)));
    if (batch < P) batch = batch / A.ob * A.ob;  // (at least 256 orders: whole blocks)

    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // one allocation: the partials (the batches take turns with them in stream order), and behind them the orders
    DevPtr<uint32_t> scratch;
    const size_t orders_n = (size_t)P * M, scratch_n = (size_t)gx * batch * M * 2, words_n = scratch_n + (orders_n + 1) / 2;
    if (hipError_t err = scratch.alloc(words_n); err != hipSuccess)
        return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the partial curves of %d orders and the orders: %s", words_n * sizeof(uint32_t), batch,
                    hipGetErrorString(err));
    uint16_t *d_orders = reinterpret_cast<uint16_t *>(scratch + scratch_n);
    HIP_TRY(hipMemcpyAsync(d_orders, orders_host, orders_n * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    A.partials = scratch;
    Laps laps(st, g_collect_timed, g_collect_ms);  // (the batches add up)
    if (g_collect_timed) g_collect_ms[0] = g_collect_ms[1] = 0.f;
    if (int rc = laps.start()) return rc;
    for (int q0 = 0; q0 < P; q0 += batch) {
        A.P = std::min(batch, P - q0);
        A.orders = d_orders + (size_t)q0 * M;
        A.core = d_core + (size_t)q0 * M;
        A.covered = d_covered + (size_t)q0 * M;
        const int gy = (A.P + A.ob - 1) / A.ob;
        if (int rc = pw == 16 ? launch_sweep<16>(A, gx, gy, lds, st) : pw == 8 ? launch_sweep<8>(A, gx, gy, lds, st) : launch_sweep<4>(A, gx, gy, lds, st))
            return rc;
        if (int rc = laps.add(0)) return rc;
        hipLaunchKernelGGL(collect_reduce_kernel, dim3((unsigned)(((int64_t)A.P * M + 15) / 16)), dim3(kThreads), 0, st, A, gx);
        HIP_TRY(hipGetLastError());
        if (int rc = laps.add(1)) return rc;
    }
    HIP_TRY(hipStreamSynchronize(st));
    return MEMO_OK;
}

}  // extern "C"
