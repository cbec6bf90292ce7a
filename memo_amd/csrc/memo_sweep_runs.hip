// memo_sweep_runs.hip -- conservation results DECODED from the run copy of one k - 1 (memo_view_build.hip: run_view_copy; the rule:
// memo_view.hip, run_rows), in the place of a sweep over the deciding copy's rows.
//
// The copy holds the answer itself: per bucket of 32 positions a start mask (bit i: result[i] differs from result[i - 1]; bit 0 always)
// and the byte offset of the bucket's first value; per run one byte -- the least order that covers it, 255: none.  A lane decodes
// kDecodeP consecutive positions of one bucket (memo_runs_decode.h): it loads its bucket's table entry, then the kDecodeP / 4 + 1 dwords
// of values from the dword that holds its first position's byte on, and picks every quartet's bytes with one v_perm_b32.  A wave takes
// 64 kDecodeP positions a turn, counted from the copy's first position.  No LDS, no cross-lane traffic, no atomics, no barrier, no halo.
// PER-LANE READ BOUND: an entry of the table inside [0, buckets) and the bytes [A & ~3, (A & ~3) + kDecodeP + 4) of the values, A < the
// copy's value_bytes: at most kDecodeP bytes past them, which the zeroed pad of run_view_copy (512 bytes) covers.  A lane whose bucket
// is outside the copy loads nothing and decodes to "no row" -- a per-lane test: the copy ends on a group of 256 positions, not on a turn.
// out = value == 255 ? num_docs : value, with the query's num_docs, not the copy's.  (min(value, num_docs) needs no instruction: the
// dense rows answer only where every order of the index is <= num_docs -- query_conservation's `checked` -- and the launcher refuses
// anything else.)
#include "memo_sweep.h"
#include "memo_runs_decode.h"

namespace memo {
namespace {

constexpr int kDecodeP = 8;                              // positions a lane decodes a turn (16: the same headline, 3 % slower at k = 17 -- profiles/run_decode.txt)
constexpr int kDecodeTurns = 4;                          // turns of a wave
constexpr int kDecodeTurn = 64 * kDecodeP;               // positions a wave decodes a turn
constexpr int kDecodeTurnBuckets = kDecodeTurn / 32;
constexpr int kDecodeSpan = kDecodeTurn * 4 * kDecodeTurns;  // positions a workgroup of four waves decodes

struct DecodeArgs {
    const uint2 *tab;      // per bucket: start mask, byte offset of its first value
    const uint32_t *vals;  // the values' bytes as dwords (kDecodeP bytes past the last are readable)
    int64_t p0;            // the pivot position of the copy's first bucket
    int64_t buckets;       // of the copy
    int64_t t_first;       // the turn (from p0; may be negative) that holds qs
    int64_t t_count;       // turns the window touches
    int64_t qs, qe;
    void *out;
    uint32_t nd;           // num_docs
    int mode;              // 0: bytes go out as they are (uint8, num_docs 255); 1: 255 -> num_docs
};

// four value bytes -> what store_four takes.  mode as DecodeArgs::mode (wave-uniform).
__device__ __forceinline__ uint32_t results_of(uint32_t R, uint32_t nd, int mode, uint8_t) {
    if (mode == 0) return R;
    // a byte is 255 where its low seven bits carry into a set top bit
    const uint32_t t = ((R & 0x7F7F7F7Fu) + 0x01010101u) & R & 0x80808080u, m = (t << 1) - (t >> 7);
    return (R & ~m) | ((nd * 0x01010101u) & m);
}
__device__ __forceinline__ uint2 results_of(uint32_t R, uint32_t nd, int mode, uint16_t) {
    const uint32_t lo = __builtin_amdgcn_perm(0u, R, 0x0c010c00u), hi = __builtin_amdgcn_perm(0u, R, 0x0c030c02u);
    const uint32_t nn = nd | (nd << 16);
    const uint32_t tl = ((lo & 0x007F007Fu) + 0x00010001u) & lo & 0x00800080u, ml = (tl << 9) - (tl >> 7);
    const uint32_t th = ((hi & 0x007F007Fu) + 0x00010001u) & hi & 0x00800080u, mh = (th << 9) - (th >> 7);
    return make_uint2((lo & ~ml) | (nn & ml), (hi & ~mh) | (nn & mh));
}
__device__ __forceinline__ void store_one(uint8_t *p, uint32_t v, int i) { p[i] = (uint8_t)(v >> (8 * i)); }
__device__ __forceinline__ void store_one(uint16_t *p, uint2 v, int i) { p[i] = (uint16_t)((i < 2 ? v.x : v.y) >> (16 * (i & 1))); }

// A lane's eight results in one store, at whatever address the window's start makes of it (memo_sweep.h: store_four): 8 bytes
// (uint8) or 16 (uint16).
static_assert(kDecodeP == 8, "store_lane stores two quartets");
typedef uint32_t __attribute__((ext_vector_type(2), aligned(1))) u32x2_any;
typedef uint32_t __attribute__((ext_vector_type(4), aligned(2))) u32x4_any;
__device__ __forceinline__ void store_lane(uint8_t *p, const uint32_t (&v)[2]) {
    u32x2_any w = {v[0], v[1]};
    *reinterpret_cast<u32x2_any *>(p) = w;
}
__device__ __forceinline__ void store_lane(uint16_t *p, const uint2 (&v)[2]) {
    u32x4_any w = {v[0].x, v[0].y, v[1].x, v[1].y};
    *reinterpret_cast<u32x4_any *>(p) = w;
}

// The turns of one wave.  FULL (wave-uniform, decided once a workgroup): every turn of the workgroup lies inside the copy and inside
// the window -- no test of any kind, one store a lane and turn.  Otherwise: a turn may lie past the window's last (it is skipped), a
// lane's bucket outside the copy (it loads nothing), and the window's first and last turn store whole quartets where they fit and
// single positions at the two edges.  All that is 64-bit is wave-uniform; per lane the offsets fit 32 bits.
template <typename OutT, bool FULL, int MODE>
__device__ __forceinline__ void decode_turns(const DecodeArgs &a, uint32_t lane, int64_t ti0) {
    constexpr int P = kDecodeP, Q = P / 4, LPB = 32 / P;   // quartets a lane, lanes a bucket
    const uint32_t lb = lane / LPB, r = (lane % LPB) * P;  // the lane's bucket inside the turn, its first position inside the bucket
    OutT *const out = static_cast<OutT *>(a.out);
    uint2 e[kDecodeTurns];
    bool in[kDecodeTurns];
    RunDwords<P> D[kDecodeTurns];
    uint32_t A[kDecodeTurns];
    // every turn's table load goes out before the first value load, which waits for its entry
#pragma unroll
    for (int t = 0; t < kDecodeTurns; ++t) {
        const int64_t b = (a.t_first + ti0 + 4 * t) * kDecodeTurnBuckets;  // the turn's first bucket
        if constexpr (FULL) {
            in[t] = true;
            e[t] = (a.tab + b)[lb];
        } else {
            in[t] = false;
            e[t] = make_uint2(1u, 0u);
            if (ti0 + 4 * t >= a.t_count) break;
            const int64_t left = a.buckets - b;  // buckets of the copy from b on
            const uint32_t nin = b < 0 || left <= 0 ? 0u : (left > kDecodeTurnBuckets ? (uint32_t)kDecodeTurnBuckets : (uint32_t)left);
            in[t] = lb < nin;
            if (in[t]) e[t] = (a.tab + b)[lb];
        }
    }
#pragma unroll
    for (int t = 0; t < kDecodeTurns; ++t) {
        if (!FULL && ti0 + 4 * t >= a.t_count) break;
        A[t] = runs_lane_first(e[t].x, e[t].y, r);
        if (FULL || in[t]) D[t] = runs_lane_load<P>(a.vals, A[t]);
    }
#pragma unroll
    for (int t = 0; t < kDecodeTurns; ++t) {
        if (!FULL && ti0 + 4 * t >= a.t_count) break;
        decltype(results_of(0u, 0u, 0, OutT())) res[Q];
        RunQuartets<P> R;
        if (FULL || in[t]) R = runs_lane_pick<P>(e[t].x, r, A[t], D[t]);
#pragma unroll
        for (int j = 0; j < Q; ++j) res[j] = results_of(FULL || in[t] ? R.q[j] : 0xFFFFFFFFu, a.nd, MODE, OutT());  // (outside the copy: no row)
        const int64_t s = a.p0 + (a.t_first + ti0 + 4 * t) * kDecodeTurn;  // the turn's first position
        OutT *const at = out + (s - a.qs);  // (before `out` in the window's first turn: nothing below qs is stored)
        const uint32_t x = lane * P;
        if (FULL || (s >= a.qs && s + kDecodeTurn <= a.qe)) {  // the whole turn lies inside the window
            store_lane(at + x, res);
            continue;
        }
        const int64_t dl = a.qs - s, dh = a.qe - s;  // (a turn of the window: dl < kDecodeTurn, dh > 0)
        const uint32_t lo = dl < 0 ? 0u : (uint32_t)dl, hi = dh > kDecodeTurn ? (uint32_t)kDecodeTurn : (uint32_t)dh;
#pragma unroll
        for (int j = 0; j < Q; ++j) {
            const uint32_t xq = x + 4u * j;
            if (xq >= lo && xq + 4u <= hi) {
                store_four(at + xq, res[j]);
            } else if (xq < hi && xq + 4u > lo) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (xq + i >= lo && xq + i < hi) store_one(at + xq, res[j], i);
            }
        }
    }
}

template <typename OutT>
__global__ __launch_bounds__(256) void decode_runs_kernel(const DecodeArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // turn t of this wave is the window's turn ti0 + 4 t: the four waves take neighbouring turns
    const int64_t w0 = (int64_t)blockIdx.x * (4 * kDecodeTurns), ti0 = w0 + wave;
    // the workgroup's turns [w0, w0 + 4 kDecodeTurns): all of the window's, of the copy's buckets and of the window's positions?
    const int64_t b_lo = (a.t_first + w0) * kDecodeTurnBuckets, s_lo = a.p0 + b_lo * 32;
    const bool full = w0 + 4 * kDecodeTurns <= a.t_count && b_lo >= 0 && b_lo + 4 * kDecodeTurns * kDecodeTurnBuckets <= a.buckets &&
                      s_lo >= a.qs && s_lo + kDecodeSpan <= a.qe;
    if (a.mode == 0) {
        if (full) decode_turns<OutT, true, 0>(a, lane, ti0);
        else decode_turns<OutT, false, 0>(a, lane, ti0);
    } else {
        if (full) decode_turns<OutT, true, 1>(a, lane, ti0);
        else decode_turns<OutT, false, 1>(a, lane, ti0);
    }
}

}  // namespace

int launch_runs_decode(memo_index *ix, const SweepArgs &A, const RowSource &src, int elem_bytes, hipStream_t st) {
    auto floor_div = [](int64_t x, int64_t d) { return x >= 0 ? x / d : -((-x + d - 1) / d); };
    DecodeArgs a;
    a.tab = reinterpret_cast<const uint2 *>(src.run_tab);
    a.vals = src.run_vals;
    a.p0 = src.run_b0 * 32;
    a.buckets = (int64_t)src.run_buckets;
    a.qs = A.qs;
    a.qe = A.qe;
    // (a window wholly off the copy by more than its own length: every turn decodes to "no row" wherever it is counted from)
    a.t_first = floor_div(A.qs - a.p0, kDecodeTurn);
    a.t_count = floor_div(A.qe - 1 - a.p0, kDecodeTurn) - a.t_first + 1;
    a.out = A.out;
    a.nd = (uint32_t)(A.ncols - 1);
    if (ix->max_annot > (uint64_t)a.nd) return fail(MEMO_EHIP, "internal: a run copy was handed to a query with orders past its num_docs");
    a.mode = elem_bytes == 1 && a.nd == 255u ? 0 : 1;
    const int64_t blocks = (a.t_count + 4 * kDecodeTurns - 1) / (4 * kDecodeTurns);
    if (blocks < 1 || blocks >= ((int64_t)1 << 31)) return fail(MEMO_EINVAL, "the window is too long for one decode launch");
    ix->last_rows_read = src.runs;
    ix->last_tile_w = kDecodeSpan;
    ix->last_tiles_per_group = 1;
    ix->last_pick.threads = 256, ix->last_pick.width = kDecodeSpan, ix->last_pick.arrays = 0, ix->last_pick.kernel = 5;
    if (g_prepare_only) return MEMO_OK;  // memo_index_prepare: nothing is launched
    if (int prc = refuse_plan_pointer(A.out)) return prc;
    if (elem_bytes == 1)
        hipLaunchKernelGGL(decode_runs_kernel<uint8_t>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(decode_runs_kernel<uint16_t>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return MEMO_OK;
}

}  // namespace memo
