// memo_sweep_fold.h -- the tail the unclipped conservation sweeps share (memo_sweep_cons.hip, memo_sweep_cons3t.hip): the fold steps in
// registers, the chunk loop around them and the store of a lane's four cells
#ifndef MEMO_SWEEP_FOLD_H
#define MEMO_SWEEP_FOLD_H

#include "memo_sweep.h"

namespace memo {

// M_(j-1)[x] = min(L[x], M_j[x], M_j[x - half]),  half = 2^J cells, on a lane's four cells, IN PLACE (one asm block
// per step: the compiler, left to itself, computes into fresh registers and copies them back at the join of the
// wave-uniform branch around the step).  The DPP operations come first -- they read the left lane's M before any
// lane overwrites it -- and fold their operand into L; s_nop 1: a DPP source written by the instruction before
// needs two wait states, and the compiler does not see into the string.
#define MEMO_DPP_MIN(dst, src) "v_min_u32_dpp " dst ", " src ", " dst " wave_shr:1 row_mask:0xf bank_mask:0xf\n\t"
#define MEMO_DPP_MOV(dst, src) "v_mov_b32_dpp " dst ", " src " wave_shr:1 row_mask:0xf bank_mask:0xf\n\t"
template <int J>
__device__ __forceinline__ void fold_step_dpp(uint4 &M, uint4 L, int lane) {
    if constexpr (J >= 3) {
        const int src = (lane - (1 << (J - 2))) << 2;  // (negative: context lanes, whose result is dropped)
        const uint32_t sx = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)M.x), sy = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)M.y);
        const uint32_t sz = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)M.z), sw = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)M.w);
        M = make_uint4(min(L.x, min(M.x, sx)), min(L.y, min(M.y, sy)), min(L.z, min(M.z, sz)), min(L.w, min(M.w, sw)));
    } else if constexpr (J == 2) {
        asm("s_nop 1\n\t" MEMO_DPP_MIN("%4", "%0") MEMO_DPP_MIN("%5", "%1") MEMO_DPP_MIN("%6", "%2") MEMO_DPP_MIN("%7", "%3")
            "v_min_u32 %0, %4, %0\n\tv_min_u32 %1, %5, %1\n\tv_min_u32 %2, %6, %2\n\tv_min_u32 %3, %7, %3"
            : "+v"(M.x), "+v"(M.y), "+v"(M.z), "+v"(M.w), "+v"(L.x), "+v"(L.y), "+v"(L.z), "+v"(L.w));
    } else if constexpr (J == 1) {
        asm("s_nop 1\n\t" MEMO_DPP_MIN("%4", "%2") MEMO_DPP_MIN("%5", "%3")
            "v_min3_u32 %2, %6, %2, %0\n\tv_min3_u32 %3, %7, %3, %1\n\tv_min_u32 %0, %4, %0\n\tv_min_u32 %1, %5, %1"
            : "+v"(M.x), "+v"(M.y), "+v"(M.z), "+v"(M.w), "+v"(L.x), "+v"(L.y) : "v"(L.z), "v"(L.w));
    } else {
        asm("s_nop 1\n\t" MEMO_DPP_MIN("%4", "%3")
            "v_min3_u32 %3, %7, %3, %2\n\tv_min3_u32 %2, %6, %2, %1\n\tv_min3_u32 %1, %5, %1, %0\n\tv_min_u32 %0, %4, %0"
            : "+v"(M.x), "+v"(M.y), "+v"(M.z), "+v"(M.w), "+v"(L.x) : "v"(L.y), "v"(L.z), "v"(L.w));
    }
}

// The radix-4 folds on a lane's four cells: operands from the lanes to the left through DPP, one in-place asm block per step.
// (memo_sweep_cons.hip kept the 16 -> 4 and 4 -> 1 steps inline for a while because, called from here, its code "came out scheduled
// differently".  It does -- the same instructions under another register allocation, at the same VGPRs, occupancy and scratch -- and
// that costs nothing: config 3, radix-4 arrays, k = 101 / 256: -0.6 / +0.04 %; the level plan's mixed arrays: +0.07 / -0.25 %, the
// parent's own rounds spreading by 0.3 .. 2.1 %.  profiles/fold_tail_refactor.txt.)
// Blocks of 16 -> blocks of 4 (the radix-4 and the mixed arrays of memo_sweep_cons.hip): cells x - 4, x - 8, x - 12 are the same
// component 1, 2, 3 lanes left.  B = min over this lane and the one to the left, in place, P = B one lane left; M = min(M, B, P one
// more lane left).  (P of lane 0: whatever was there; a context lane, like lanes 1 .. 3.)
__device__ __forceinline__ void r4_fold16(uint4 &M, uint4 B) {
    uint4 P;
    asm("s_nop 1\n\t" MEMO_DPP_MIN("%4", "%4") MEMO_DPP_MIN("%5", "%5") MEMO_DPP_MIN("%6", "%6") MEMO_DPP_MIN("%7", "%7")
        MEMO_DPP_MOV("%8", "%4") MEMO_DPP_MOV("%9", "%5") MEMO_DPP_MOV("%10", "%6") MEMO_DPP_MOV("%11", "%7")
        "v_min_u32 %0, %4, %0\n\tv_min_u32 %1, %5, %1\n\tv_min_u32 %2, %6, %2\n\tv_min_u32 %3, %7, %3\n\t"
        MEMO_DPP_MIN("%0", "%8") MEMO_DPP_MIN("%1", "%9") MEMO_DPP_MIN("%2", "%10") MEMO_DPP_MIN("%3", "%11")
        : "+v"(M.x), "+v"(M.y), "+v"(M.z), "+v"(M.w), "+v"(B.x), "+v"(B.y), "+v"(B.z), "+v"(B.w),
          "=&v"(P.x), "=&v"(P.y), "=&v"(P.z), "=&v"(P.w));
}

// Blocks of 12 -> blocks of 4 (the six-row views' wide tiles, memo_sweep_cons3t.hip: R4): a block of 12 is three blocks of 4, at cells
// x, x - 4 and x - 8 -- the same component of this lane and of the two to its left.  B as above; M = min(M, B, B one lane left).
// (Lane 0 keeps what it had, lane 1 lacks its second neighbour: context lanes.)
__device__ __forceinline__ void r4_fold12(uint4 &M, uint4 B) {
    asm("s_nop 1\n\t" MEMO_DPP_MIN("%4", "%4") MEMO_DPP_MIN("%5", "%5") MEMO_DPP_MIN("%6", "%6") MEMO_DPP_MIN("%7", "%7")
        "v_min_u32 %0, %4, %0\n\tv_min_u32 %1, %5, %1\n\tv_min_u32 %2, %6, %2\n\tv_min_u32 %3, %7, %3\n\t"
        MEMO_DPP_MIN("%0", "%4") MEMO_DPP_MIN("%1", "%5") MEMO_DPP_MIN("%2", "%6") MEMO_DPP_MIN("%3", "%7")
        : "+v"(M.x), "+v"(M.y), "+v"(M.z), "+v"(M.w), "+v"(B.x), "+v"(B.y), "+v"(B.z), "+v"(B.w));
}

// blocks of 4 -> positions: cell x takes the blocks at x, x - 1, x - 2, x - 3 (the last ones of the lane to the left)
__device__ __forceinline__ void r4_fold4(uint4 &R, uint4 M) {
    asm("s_nop 1\n\t"
        "v_min3_u32 %3, %3, %7, %6\n\tv_min3_u32 %3, %3, %5, %4\n\t"
        "v_min3_u32 %2, %2, %6, %5\n\tv_min_u32 %2, %2, %4\n\t"
        "v_min3_u32 %1, %1, %5, %4\n\tv_min_u32 %0, %0, %4\n\t"
        MEMO_DPP_MIN("%2", "%7") MEMO_DPP_MIN("%1", "%7") MEMO_DPP_MIN("%0", "%7")
        MEMO_DPP_MIN("%1", "%6") MEMO_DPP_MIN("%0", "%6") MEMO_DPP_MIN("%0", "%5")
        : "+v"(R.x), "+v"(R.y), "+v"(R.z), "+v"(R.w) : "v"(M.x), "v"(M.y), "v"(M.z), "v"(M.w));
}
#undef MEMO_DPP_MIN
#undef MEMO_DPP_MOV

// What every level cell starts at: the sentinel column N (memo_query.py:53-54).  TOP != 0: the cells hold whole row words whose bits
// from TOP up are the order -- the sentinel on top, all ones below it.
template <int TOP>
__device__ __forceinline__ uint32_t cell_sentinel(int ncols) {
    const uint32_t sent = (uint32_t)(ncols - 1);
    return TOP ? (sent << TOP) | ((1u << TOP) - 1u) : sent;
}
template <int TOP>
__device__ __forceinline__ uint32_t cell_sentinel(const SweepArgs &A) {
    return cell_sentinel<TOP>(A.ncols);
}

// A lane's four cells to results g .. g + 3 of the window [o_lo, o_hi): one store for a whole quartet (at whatever address the window's
// start makes of it: store_four), cell by cell at the window's edges
template <typename OutT, int TOP>
__device__ __forceinline__ void store_cells4(OutT *out, int64_t g, int64_t o_lo, int64_t o_hi, uint4 R) {
    if (g >= o_lo && g + 4 <= o_hi) {
        store_four(out + g, pack_cells4<OutT, TOP>(R));
    } else {
        const uint32_t v[4] = {R.x >> TOP, R.y >> TOP, R.z >> TOP, R.w >> TOP};
        for (int i = 0; i < 4; ++i)
            if (g + i >= o_lo && g + i < o_hi) out[g + i] = (OutT)v[i];
    }
}

// The chunk loop of the register folds.  A wave walks the level arrays (`cells` cells in use, LS allocated) in chunks of 64 lanes, four
// cells per lane; fold(xr) reads the lane's cells xr .. xr + 3 of every level (xr clamped into the array: past it sit lanes whose
// result is dropped) and returns them folded.  The leftmost `ctx` lanes of a chunk only supply context to the lanes right of them --
// their own results would need cells of the chunk before -- so consecutive chunks overlap by that much; chunk 0's context lanes hold the
// first cells of the left halo, whose results nobody stores and left of which no block can start.  ob: output index of cell 0.
// lane, wave: where the thread sits in its workgroup, as the kernel already holds them (the table-driven kernel's wave number is in
// an SGPR).  ctx: an int, or an Int<> where the kernel knows it at compile time.  (The table-driven kernel's doubling arrays keep
// this loop written out: memo_sweep_cons3t.hip says why.)
template <typename OutT, int T, int TOP, typename Ctx, typename Fold>
__device__ __forceinline__ void fold_store_chunks(OutT *out, int64_t ob, int64_t o_lo, int64_t o_hi, int cells, int LS, int lane,
                                                  int wave, Ctx ctx, Fold fold) {
    constexpr int NW = T / 64;
    const int valid = 64 - ctx;
    for (int base = wave * 4 * valid; base + 4 * ctx < cells; base += NW * 4 * valid) {
        const int x0 = base + 4 * lane;  // this lane's cells x0 .. x0 + 3
        const uint4 R = fold(min(x0, LS - 4));
        if (lane < ctx || x0 >= cells) continue;
        store_cells4<OutT, TOP>(out, ob + x0, o_lo, o_hi, R);
    }
}

// The same walk for a kernel whose waves have at most two chunks (the wide tiles of memo_sweep_cons3t.hip), with the store handed in:
// store(x0, R) gets the four folded cells of every lane that is no context lane and lies inside the cells in use.  TWO: a wave with
// two chunks has both in flight -- fold2(xa, xb, Ra, Rb) reads both chunks' levels, waits once and folds both (the chunks share no
// cell a fold writes; the LDS round trip of the second is not paid behind the first's fold and store).  A wave with one chunk, and
// every wave without TWO, goes chunk by chunk through fold1 as above.
template <int T, bool TWO, typename Ctx, typename Fold1, typename Fold2, typename Store>
__device__ __forceinline__ void fold_chunks_once_or_twice(int cells, int LS, int lane, int wave, Ctx ctx, Fold1 fold1, Fold2 fold2,
                                                          Store store) {
    constexpr int NW = T / 64;
    const int valid = 64 - ctx, step = NW * 4 * valid;
    const int base = wave * 4 * valid;
    if (TWO && base + step + 4 * ctx < cells) {  // (wave-uniform.  Both chunks begin inside the array; only the second can leave it)
        const int x0 = base + 4 * lane, x1 = x0 + step;
        uint4 Ra, Rb;
        fold2(x0, min(x1, LS - 4), Ra, Rb);
        if (lane < ctx) return;
        store(x0, Ra);
        if (x1 < cells) store(x1, Rb);
        return;
    }
    for (int b = base; b + 4 * ctx < cells; b += step) {
        const int x0 = b + 4 * lane;
        const uint4 R = fold1(min(x0, LS - 4));
        if (lane < ctx || x0 >= cells) continue;
        store(x0, R);
    }
}

}  // namespace memo

#endif  // MEMO_SWEEP_FOLD_H
