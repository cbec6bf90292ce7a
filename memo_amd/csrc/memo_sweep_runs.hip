// memo_sweep_runs.hip -- conservation results DECODED from the run copy of one k - 1 (memo_view_build.hip: run_view_copy; the rule:
// memo_view.hip, run_rows), in the place of a sweep over the deciding copy's rows.
//
// The copy holds the answer itself: per bucket of 32 positions a start mask (bit i: result[i] differs from result[i - 1]; bit 0 always)
// and the byte offset of the bucket's first value; per run one byte -- the least order that covers it, 255: none.  A group of kRunGroup
// buckets (256 positions) has its values at a multiple of four bytes, at most 256 of them.  So a wave takes a group a turn: every lane
// loads one dword of the group's values (64 dwords hold the most a group can need) and its bucket's table entry; a lane's four positions
// want four bytes at non-decreasing indices that span at most two dwords, which come through ds_bpermute_b32 and are picked by one
// v_perm_b32; one 4- / 8-byte store a lane.  No LDS arrays, no atomics, no barrier, no halo.  A group outside the copy decodes to "no row".
// out = value == 255 ? num_docs : value, with the query's num_docs, not the copy's.  (min(value, num_docs) needs no instruction: the
// dense rows answer only where every order of the index is <= num_docs -- query_conservation's `checked` -- and the launcher refuses
// anything else.)
#include "memo_sweep.h"

namespace memo {
namespace {

constexpr int kDecodeTurns = 4;                          // groups a wave decodes
constexpr int kDecodeSpan = 256 * 4 * kDecodeTurns;      // positions a workgroup of four waves decodes

struct DecodeArgs {
    const uint2 *tab;      // per bucket: start mask, byte offset of its first value
    const uint32_t *vals;  // the values' bytes as dwords (64 dwords past a group's first are readable)
    int64_t p0;            // the pivot position of the copy's first bucket
    int64_t groups;        // of the copy
    int64_t g_first;       // the group (from p0; may be negative) that holds qs
    int64_t g_count;       // groups the window touches
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

template <typename OutT>
__global__ __launch_bounds__(256) void decode_runs_kernel(const DecodeArgs a) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    OutT *const out = static_cast<OutT *>(a.out);
#pragma unroll
    for (int t = 0; t < kDecodeTurns; ++t) {
        const int64_t gi = ((int64_t)blockIdx.x * kDecodeTurns + t) * 4 + wave;  // (wave-uniform, like all that decides a branch before the store)
        if (gi >= a.g_count) break;
        const int64_t g = a.g_first + gi;
        uint32_t R = 0xFFFFFFFFu;  // (outside the copy: no row)
        if (g >= 0 && g < a.groups) {
            const uint2 e = a.tab[g * kRunGroup + (lane >> 3)];  // the lane's bucket: its mask, its first value
            const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)e.y);  // the group's first value: a multiple of four
            const uint32_t d = a.vals[(first >> 2) + lane];
            const uint32_t r = (lane & 7u) * 4u;  // the lane's first position inside its bucket
            const uint32_t i0 = e.y - first + (uint32_t)__popc(e.x & ((2u << r) - 1u)) - 1u;  // the byte of that position, from `first`: 0 .. 255
            const uint32_t steps = (((e.x >> (r + 1)) & 7u) * 0x408100u) & 0x01010100u;  // the next three start bits, one to a byte
            const uint32_t w0 = i0 >> 2, w1 = w0 < 63u ? w0 + 1u : 63u;
            const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(w0 << 2), (int)d);
            const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(w1 << 2), (int)d);
            uint32_t sel = (i0 & 3u) * 0x01010101u + steps;  // byte i: where position i's value lies in hi:lo (at most 3 + 3)
            sel += steps << 8;
            sel += (steps & 0x0100u) << 16;
            R = __builtin_amdgcn_perm(hi, lo, sel);
        }
        const int64_t p = a.p0 + g * 256 + 4 * (int64_t)lane;
        if (p >= a.qe || p + 4 <= a.qs) continue;
        const auto four = results_of(R, a.nd, a.mode, OutT());
        OutT *const at = out + (p - a.qs);
        if (p >= a.qs && p + 4 <= a.qe) {
            store_four(at, four);
        } else {  // (the window's first and last quartet)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (p + i >= a.qs && p + i < a.qe) store_one(at, four, i);
        }
    }
}

}  // namespace

int launch_runs_decode(memo_index *ix, const SweepArgs &A, const RowSource &src, int elem_bytes, hipStream_t st) {
    auto floor_div = [](int64_t x, int64_t d) { return x >= 0 ? x / d : -((-x + d - 1) / d); };
    DecodeArgs a;
    a.tab = reinterpret_cast<const uint2 *>(src.run_tab);
    a.vals = src.run_vals;
    a.p0 = src.run_b0 * 32;
    a.groups = (int64_t)(src.run_buckets / kRunGroup);
    a.qs = A.qs;
    a.qe = A.qe;
    // (a window wholly off the copy by more than its own length: every group decodes to "no row" wherever it is counted from)
    a.g_first = floor_div(A.qs - a.p0, 256);
    a.g_count = floor_div(A.qe - 1 - a.p0, 256) - a.g_first + 1;
    a.out = A.out;
    a.nd = (uint32_t)(A.ncols - 1);
    if (ix->max_annot > (uint64_t)a.nd) return fail(MEMO_EHIP, "internal: a run copy was handed to a query with orders past its num_docs");
    a.mode = elem_bytes == 1 && a.nd == 255u ? 0 : 1;
    const int64_t blocks = (a.g_count + 4 * kDecodeTurns - 1) / (4 * kDecodeTurns);
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
