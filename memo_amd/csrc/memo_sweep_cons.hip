// memo_sweep_cons.hip -- conservation sweep: doubling scatter + top-down fold, the
// k <= 1 fill, the side pass for rows with end < start, tile-shape choice and the ABI entry points.
// Replaces /root/reference/src/memo_query.py:42-63 + the argmax of :70.
#include "memo_sweep.h"
#include "memo_sweep_fold.h"

using namespace memo;

namespace {

// ------------------------------------------------------------------------------------------
// conservation: doubling scatter + top-down fold
// ------------------------------------------------------------------------------------------
template <typename Rows, int W, int U, int T, typename OutT>
__global__ __launch_bounds__(T) void sweep_conservation_kernel(const SweepArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int tid = threadIdx.x;
    constexpr int LS = W;  // words between level arrays
    Tile t;
#ifdef MEMO_STAMPS
    unsigned long long stamp_t0 = __builtin_amdgcn_s_memtime();
#endif
    if (!locate_tile<W>(A, t)) return;
    MEMO_STAMP(0);  // tile location (kernarg + two bucket-table loads)

    // the clipped interval [c, h) is the union of two blocks of 2^j, j = floor(log2(h - c))
    Rows::template for_each<T, U>(
        A, t,
        [&]() {  // every level starts at the sentinel column N (memo_query.py:53-54)
            const uint32_t sent = (uint32_t)(A.ncols - 1);
            const uint4 sv = make_uint4(sent, sent, sent, sent);
            uint4 *p = reinterpret_cast<uint4 *>(lds);
            for (int i = tid; i < A.nlev * (LS / 4); i += T) p[i] = sv;
            lds_barrier();
            MEMO_STAMP(1);  // issue of the first loads + LDS clear + barrier
        },
        [&](int c, int h, int col) {
            if (h > c) {
                const int j = 31 - __builtin_clz((unsigned)(h - c));  // h - c >= 1
                uint32_t *lv = lds + j * LS;
                atomicMin(lv + c, (uint32_t)col);               // block [c, c + 2^j)
                atomicMin(lv + (h - (1 << j)), (uint32_t)col);  // block [h - 2^j, h)
            }
        });
    MEMO_STAMP(2);  // waiting for rows + scatter
    __syncthreads();
    MEMO_STAMP(3);  // barrier after the scatter

    // fold: a block of 2^j at x covers the blocks of 2^(j-1) at x and x + 2^(j-1)
    for (int j = A.nlev - 1; j >= 2; --j) {  // (level 1 -> 0 happens in store_conservation)
        const int half = 1 << (j - 1);
        const uint32_t *hi = lds + j * LS;
        uint32_t *lo = lds + (j - 1) * LS;
        for (int x = 4 * tid; x < W; x += 4 * T) {
            const uint4 v = *reinterpret_cast<const uint4 *>(hi + x);
            uint4 u;
            if (half >= 4) {
                u = x >= half ? *reinterpret_cast<const uint4 *>(hi + x - half)
                              : make_uint4(~0u, ~0u, ~0u, ~0u);
            } else if (half == 2) {
                const uint2 q = x >= 2 ? *reinterpret_cast<const uint2 *>(hi + x - 2)
                                       : make_uint2(~0u, ~0u);
                u = make_uint4(q.x, q.y, v.x, v.y);
            } else {
                const uint32_t q = x >= 1 ? hi[x - 1] : ~0u;
                u = make_uint4(q, v.x, v.y, v.z);
            }
            uint4 w = *reinterpret_cast<const uint4 *>(lo + x);
            w.x = min(w.x, min(v.x, u.x));
            w.y = min(w.y, min(v.y, u.y));
            w.z = min(w.z, min(v.z, u.z));
            w.w = min(w.w, min(v.w, u.w));
            *reinterpret_cast<uint4 *>(lo + x) = w;
        }
        __syncthreads();
    }

    MEMO_STAMP(4);  // fold
    store_conservation<OutT, T>(A, t, lds, A.nlev > 1 ? lds + LS : nullptr, 0);  // as uint16 or (num_docs <= 255) uint8
    MEMO_STAMP(5);  // store
#ifdef MEMO_STAMPS
    if (threadIdx.x == 0 && A.stamps) A.stamps[8ull * blockIdx.x + 7] = 1;
#endif
}


// ------------------------------------------------------------------------------------------
// conservation, packed rows whose annot is known to be inside the matrix: the same doubling scatter
// WITHOUT clipping.
//
// Every level array carries a halo -- HL cells left of the tile, HR right of it -- wide enough for
// any interval a row of the slice can have (start - a in [0, W + k - 1 + bucket - 2], length n = k - 1 -
// overlap in [1, k - 1]); what falls into the right halo is never read back, the left halo is
// folded like the rest (a block that starts left of the tile can cover tile positions).  With
// nothing to clip, the level and both cells follow from n and start - a alone: 10 VALU
// instructions per row instead of 17, and 60 VGPRs instead of 70 (8 waves per SIMD).  Levels are
// stored by leading-zero count (slot = clz(n) - clz(k - 1)): slot 0 = longest blocks.  The tile
// width W = A.w is what leaves the level array (HL + W + HR) at a round size; it is a multiple of
// the bucket width, not a power of two.
// (Measured and dropped, profiles/r01_unclipped_scatter.txt: a workgroup walking 2..32 tiles with
// the next tile's rows in flight under the fold -- 6-17 % slower than one tile per workgroup.)
// ------------------------------------------------------------------------------------------
// every level starts at the sentinel column N (memo_query.py:53-54); under the first loads
template <int T>
__device__ __forceinline__ void halo_clear(const SweepArgs &A, uint32_t *lds, uint32_t sent) {
    const uint4 sv = make_uint4(sent, sent, sent, sent);
    uint4 *p = reinterpret_cast<uint4 *>(lds);
    for (int i = threadIdx.x; i < A.nlev * (A.ls / 4); i += T) p[i] = sv;
    lds_barrier();
}

// fold: a block of 2^j at x covers the blocks of 2^(j-1) at x and x + 2^(j-1); the left halo too.
// Then the last fold + store (store_conservation).
template <typename OutT, int T, int TOP>
__device__ __forceinline__ void halo_fold_store(const SweepArgs &A, const Tile &t, uint32_t *lds) {
    const int LS = A.ls, HL = A.hl, W = A.w;
    const int cells = HL + W;
    for (int slot = 0; slot + 2 < A.nlev; ++slot) {  // (the last fold happens in store_conservation)
        const int half = 1 << (A.nlev - 2 - slot);
        const uint32_t *hi = lds + slot * LS;
        uint32_t *lo = lds + (slot + 1) * LS;
        for (int x = 4 * threadIdx.x; x < cells; x += 4 * T) {
            const uint4 v = *reinterpret_cast<const uint4 *>(hi + x);
            uint4 u;
            if (half >= 4) {
                u = x >= half ? *reinterpret_cast<const uint4 *>(hi + x - half)
                              : make_uint4(~0u, ~0u, ~0u, ~0u);
            } else if (half == 2) {
                const uint2 q = x >= 2 ? *reinterpret_cast<const uint2 *>(hi + x - 2)
                                       : make_uint2(~0u, ~0u);
                u = make_uint4(q.x, q.y, v.x, v.y);
            } else {
                const uint32_t q = x >= 1 ? hi[x - 1] : ~0u;
                u = make_uint4(q, v.x, v.y, v.z);
            }
            uint4 r = *reinterpret_cast<const uint4 *>(lo + x);
            r.x = min(r.x, min(v.x, u.x));
            r.y = min(r.y, min(v.y, u.y));
            r.z = min(r.z, min(v.z, u.z));
            r.w = min(r.w, min(v.w, u.w));
            *reinterpret_cast<uint4 *>(lo + x) = r;
        }
        lds_barrier();
    }
    store_conservation<OutT, T, TOP>(A, t, lds + (A.nlev - 1) * LS + HL,
                                      A.nlev > 1 ? lds + (A.nlev - 2) * LS + HL : nullptr, -HL);
}

// The same folds, in registers.  Every level is read ONCE (one conflict-free ds_read_b128 per lane and level) and
// the cascade  M_top = L_top,  M_(j-1)[x] = min(L_(j-1)[x], M_j[x], M_j[x - 2^(j-1)])  runs on a lane's four cells
// with the shifted operand taken from the lanes to its left: through the DPP operand of v_min_u32 itself for one
// lane, through ds_bpermute (the LDS crossbar, no bank access) for more; the result goes straight to the output.
// No intermediate level is written back and no barrier separates the steps.  The leftmost 2^(nlev-3) lanes of a chunk
// of 64 only supply context; the walk over the arrays in chunks that overlap by that much, the drop of those lanes
// and the store of the rest (any window: store_four takes the address as it comes) are fold_store_chunks, which the
// radix-4, the mixed and the table-driven sweeps share (memo_sweep_fold.h) -- every lane reads real cells, no ds_read
// is conditional.
// History (profiles/r02_fold_in_registers.txt): the compiler's rendering of this fold (lane_shr1() + min3: a copy,
// a v_mov_dpp and a share of a min3 per shifted operand, all-ones stand-ins for lanes left of the array) took
// ~100 VALU instructions per wave at k = 31 -- 30 % of a sweep whose VALU is 70 % busy -- and lost to the LDS
// passes from six levels up; written as below it takes ~40, is 2-5 % of the whole sweep faster at k = 21 / 31,
// and wins up to seven levels (k = 64: 0.53 -> 0.48 ms; k = 101 / 128 on doubling arrays: -2 / -3 %).
// (fold_step_dpp<J>: memo_sweep_fold.h)
template <typename OutT, int T, int TOP>
__device__ __forceinline__ void halo_fold_store_dpp(const SweepArgs &A, const Tile &t, const uint32_t *lds) {
    const int LS = A.ls, HL = A.hl, W = A.w, nlev = A.nlev;
    const int cells = HL + W;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ctx = nlev <= 1 ? 0 : (nlev <= 3 ? 1 : 1 << (nlev - 3));  // context lanes at the left of a chunk
    OutT *out = static_cast<OutT *>(A.out);
    const int64_t ob = t.a - A.qs - HL;  // output index of cell 0
    const int64_t o_lo = t.a - A.qs + t.x_lo, o_hi = t.a - A.qs + t.x_hi;
    fold_store_chunks<OutT, T, TOP>(out, ob, o_lo, o_hi, cells, LS, lane, wave, ctx, [&](int xr) {
        const uint32_t *p = lds + xr;
        uint4 M = *reinterpret_cast<const uint4 *>(p);
        // blocks of 2^J fold in when that level exists (wave-uniform branches around straight-line steps)
        if (nlev >= 7) fold_step_dpp<5>(M, *reinterpret_cast<const uint4 *>(p + (nlev - 6) * LS), lane);
        if (nlev >= 6) fold_step_dpp<4>(M, *reinterpret_cast<const uint4 *>(p + (nlev - 5) * LS), lane);
        if (nlev >= 5) fold_step_dpp<3>(M, *reinterpret_cast<const uint4 *>(p + (nlev - 4) * LS), lane);
        if (nlev >= 4) fold_step_dpp<2>(M, *reinterpret_cast<const uint4 *>(p + (nlev - 3) * LS), lane);
        if (nlev >= 3) fold_step_dpp<1>(M, *reinterpret_cast<const uint4 *>(p + (nlev - 2) * LS), lane);
        if (nlev >= 2) fold_step_dpp<0>(M, *reinterpret_cast<const uint4 *>(p + (nlev - 1) * LS), lane);
        return M;
    });
}

template <typename OutT, int T, int TOP>
__device__ __forceinline__ void halo_finish(const SweepArgs &A, const Tile &t, uint32_t *lds) {
    constexpr int kFoldDppLevels = 7;  // most levels folded in registers (<= 7: 2^(levels - 3) context lanes per wave)
    if (A.nlev <= kFoldDppLevels)  // (any window: store_four takes the address as it comes)
        halo_fold_store_dpp<OutT, T, TOP>(A, t, lds);
    else
        halo_fold_store<OutT, T, TOP>(A, t, lds);
}

// The row loops below run every row as ONE branch-free block: v_cmpx puts "this row writes" (n > 0) into EXEC itself,
// the address arithmetic and both ds_min run on those lanes only, and an s_mov restores EXEC (every lane of a wave
// is active in a row loop: rows outside the slice arrive as rows that cannot write).  The compiler's form of the
// same test -- v_cmp, s_and_saveexec, s_cbranch_execz, ..., s_or -- costs three scalar instructions and a branch
// per row, and the CU's one scalar unit was as busy as its vector pipes (1.3e8 SALU against 1.5e8 VALU
// wave-instructions per launch): dense rows, sustained, k = 21 / 31 / 64: 0.3218 -> 0.3133, 0.3249 -> 0.318,
// 0.383 -> 0.374 ms (profiles/r02_dense_rows_ab.txt).

// 4- and 6-byte rows.  The 4-byte rows carry their order in the top byte of the word, and the cells
// take the WORD (ds_min_u32 of the row as it was loaded: the min of the words has the min order on
// top, the junk below it only breaks ties) -- one VALU instruction per row less than extracting it;
// the store keeps the top bits (TOP = 24 / 20; needs num_docs to fit the field for the sentinel).  Otherwise the cells
// hold the order itself: the word's top byte shifted down, or the 16-bit order column.
template <typename Rows, int U, int T, typename OutT, int TOP>
__global__ __launch_bounds__(T) __attribute__((amdgpu_waves_per_eu(8, 8)))
void sweep_conservation_halo_kernel(const SweepArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    static_assert(TOP == 0 || (!Rows::kAnnot16 && TOP == Rows::kTopShift), "the order rides in the word only in the 4-byte formats");
    const int LS = A.ls, HL = A.hl, W = A.w;
    Tile t;
#ifdef MEMO_STAMPS
    unsigned long long stamp_t0 = __builtin_amdgcn_s_memtime();
#endif
    if (!locate_tile_w(A, t, W)) return;
    MEMO_STAMP(0);  // tile location (kernarg + two bucket-table loads)
    uint4 V[U];
    uint2 N[U];
    Rows::template issue<T, U>(A, t, 0, V, N);
    halo_clear<T>(A, lds, cell_sentinel<TOP>(A));
    MEMO_STAMP(1);  // issue of the loads + LDS clear + barrier

    const int km1 = A.km1;
    // LDS byte address of tile slot x on the level with clz(n) = f:  base + 4 * ((f - fmin) * LS + HL + x)
    const uint32_t ls4 = 4u * (uint32_t)LS;
    const uint32_t lds_base = (uint32_t)(size_t)(__attribute__((address_space(3))) uint32_t *)lds;
    const uint32_t bias4 = pin_vgpr((int)(lds_base + 4u * (uint32_t)HL - (uint32_t)(32 - A.nlev) * ls4));
    const uint32_t top_bit = pin_vgpr((int)0x80000000u);
    const uint32_t key = pin_vgpr((int)Rows::tile_key(t.a));
    auto scatter = [&](uint32_t w, uint32_t col) {  // n, the test, start - a, the two cells, both ds_min: one block
        uint32_t r0, r1, r2, nn;
        MEMO_EXEC_ALL_ONES(A.status);
#define MEMO_HALO_BLOCK(LEN_SEL, REL_START)                                                                           \
        asm volatile(                                                                                                \
            "v_sub_u32_sdwa %[n], %[km1], %[w] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD " LEN_SEL "\n\t"    \
            "v_cmpx_lt_i32 vcc, 0, %[n]\n\t"                                                                         \
            REL_START                                                                                                \
            "v_ffbh_u32 %[f], %[n]\n\t"                                                                              \
            "v_mad_u32_u24 %[a2], %[f], %[ls4], %[bias4]\n\t"                                                        \
            "v_lshl_add_u32 %[a2], %[rel], 2, %[a2]\n\t"                                                             \
            "v_mad_i32_i24 %[rel], %[n], -4, %[a2]\n\t"                                                              \
            "v_ashrrev_i32 %[f], %[f], %[top_bit]\n\t"                                                               \
            "v_lshl_add_u32 %[a2], %[f], 2, %[a2]\n\t"                                                               \
            "ds_min_u32 %[rel], %[data]\n\t"                                                                         \
            "ds_min_u32 %[a2], %[data]\n\t"                                                                          \
            "s_mov_b64 exec, -1"                                                                                     \
            : [f] "=&v"(r0), [rel] "=&v"(r1), [a2] "=&v"(r2), [n] "=&v"(nn)                                          \
            : [w] "v"(w), [km1] "s"(km1), [key] "v"(key), [ls4] "s"(ls4), [bias4] "v"(bias4), [top_bit] "v"(top_bit), \
              [data] "v"(TOP ? w : col)                                                                              \
            : "memory", "vcc")
        if constexpr (!Rows::kW12)
            MEMO_HALO_BLOCK(MEMO_ROW8_LEN_SEL, MEMO_ROW8_REL_START);
        else
            MEMO_HALO_BLOCK(MEMO_ROW12_LEN_SEL, MEMO_ROW12_REL_START);
#undef MEMO_HALO_BLOCK
    };
    // (batch 0, then the rest: written out in each of the four kernels.  Behind one shared helper the doubling kernels came out
    // waiting for all of a tile's rows -- s_waitcnt vmcnt(0) -- before the clear of the level arrays: profiles/fold_tail_device_code.txt)
    Rows::template consume<T, U>(A, t, 0, V, N, scatter);
    for (uint32_t b = 1, nb = Rows::template batches<T, U>(t); b < nb; ++b) {  // a dense tile: the rest
        Rows::template issue<T, U>(A, t, b, V, N);
        Rows::template consume<T, U>(A, t, b, V, N, scatter);
    }
    MEMO_STAMP(2);  // waiting for rows + scatter
    lds_barrier();  // waits for lgkmcnt(0): the ds_min above are invisible to the compiler
    MEMO_STAMP(3);  // barrier after the scatter
    halo_finish<OutT, T, TOP>(A, t, lds);
    MEMO_STAMP(5);  // folds + store
#ifdef MEMO_STAMPS
    if (threadIdx.x == 0 && A.stamps) A.stamps[8ull * blockIdx.x + 7] = 1;
#endif
}

// The same sweep on the dense rows (PackedRows3: five rows per 16 bytes; k - 1 <= 63, level arrays of at most
// 1024 cells).  Per row: 16-bit subtract (start - a, length untouched below it), and, subtract, compare | ffbh,
// bfe, mad, lshl_add, mad, ashr, lshl_add, ds_min x 2 (four rows of five as they were loaded -- the dword is the
// ds_min operand; the fifth after a v_perm_b32 and a shift).
// Where it stands (profiles/r02_dense_rows_ab.txt): back to back -- the device settled at its power cap -- this kernel
// takes 0.324 ms on config 3 where the 4-byte kernel takes 0.374 (another device: 0.331 against 0.343): 19 % fewer bytes,
// 13 % less time; what keeps it from the full 19 % is the power cap (1370 W of 1400 at 2.2 GHz; the 4-byte kernel
// runs at 2.36 GHz), i.e. what it executes per row.  Moving the arithmetic out of the row loop into a per-tile table
// indexed by the length (64 entries of two LDS offsets: 4 VALU per row fewer, one ds_read_b64 more) made it slower
// (0.46 ms: every row then waits for an LDS round trip).
template <int U, int T, typename OutT, bool A9 = false>
__global__ __launch_bounds__(T) __attribute__((amdgpu_waves_per_eu(8, 8)))
void sweep_conservation_halo3_kernel(const SweepArgs A) {
    static_assert(!A9 || sizeof(OutT) == 2, "more than 255 genomes: uint16 results");
    constexpr int TOP = A9 ? 23 : 24;  // a cell = order << TOP | tie-breaking bits
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    using Rows = PackedRows3;
    const int LS = A.ls, HL = A.hl, W = A.w;
    Tile t;
    if (!locate_tile_w(A, t, W)) return;
    uint4 V[U];
    Rows::template issue<T, U>(A, t, 0, V);
    halo_clear<T>(A, lds, cell_sentinel<TOP>(A));

    const int km1 = A.km1;
    const uint32_t ls4 = 4u * (uint32_t)LS;
    const uint32_t lds_base = (uint32_t)(size_t)(__attribute__((address_space(3))) uint32_t *)lds;
    const uint32_t bias4 = pin_vgpr((int)(lds_base + 4u * (uint32_t)HL - (uint32_t)(32 - A.nlev) * ls4));
    const uint32_t top_bit = pin_vgpr((int)0x80000000u);
    const uint32_t a10s = pin_vgpr((int)(((uint32_t)t.a & 1023u) << 6));
    // b: the row's B field in its low half, data: a word with the row's order in its top byte.  The 16-bit subtract leaves
    // r = (start - a) mod 2^10 << 6 | length, high half zero.
    auto g = [&](uint32_t b, uint32_t data) {
        // the whole row in one block, no branch: v_cmpx puts "this row writes" into EXEC itself, everything after it
        // runs on those lanes only, s_mov restores EXEC (every lane of the wave is active in the row loop)
        uint32_t r0, r1, r2, r3;
        MEMO_EXEC_ALL_ONES(A.status);
        asm volatile(
            "v_sub_u16 %3, %4, %5\n\t"
            "v_and_b32 %0, 63, %3\n\t"
            "v_sub_u32 %0, %6, %0\n\t"
            "v_cmpx_lt_i32 vcc, 0, %0\n\t"
            "v_ffbh_u32 %1, %0\n\t"
            "v_bfe_u32 %3, %3, 6, 10\n\t"
            "v_mad_u32_u24 %2, %1, %7, %8\n\t"
            "v_lshl_add_u32 %2, %3, 2, %2\n\t"
            "v_mad_i32_i24 %3, %0, -4, %2\n\t"
            "v_ashrrev_i32 %1, %1, %9\n\t"
            "v_lshl_add_u32 %2, %1, 2, %2\n\t"
            "ds_min_u32 %3, %10\n\t"
            "ds_min_u32 %2, %10\n\t"
            "s_mov_b64 exec, -1"
            : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3)
            : "v"(b), "v"(a10s), "s"(km1), "s"(ls4), "v"(bias4), "v"(top_bit), "v"(data)
            : "memory", "vcc");
    };
    Rows::template consume<T, U, decltype(g), A9>(A, t, 0, V, g);
    for (uint32_t b = 1, nb = Rows::template batches<T, U>(t); b < nb; ++b) {  // a dense tile: the rest
        Rows::template issue<T, U>(A, t, b, V);
        Rows::template consume<T, U, decltype(g), A9>(A, t, b, V, g);
    }
    lds_barrier();  // waits for lgkmcnt(0): the ds_min above are invisible to the compiler
    halo_finish<OutT, T, TOP>(A, t, lds);
}

// ------------------------------------------------------------------------------------------
// conservation, unclipped, RADIX-4 levels: blocks of 1, 4, 16, 64 positions.
//
// Doubling levels cost 4 bytes of LDS per position and level -- 28 B at k = 101, 32 B at k = 256 -- and one
// fold step per level; at large k those folds and the k-1 halo of short tiles are what the sweep spends its
// time on (profiles/r02_ablation.txt: fold passes 0.11 of 0.63 ms at k = 101).  With levels a factor FOUR
// apart there are four arrays for any k <= 256: an interval of n positions, 4^i <= n < 4^(i+1), is covered
// by blocks of S = 4^i at start - n and start - S, plus one at start - n + S when n > 2S and one at
// start - n + 2S when n > 3S (2 - 4 ds_min per row instead of 2), and a block of 4S folds into the four
// blocks of S under it.  Tiles are twice as long in the same LDS, the halo's share of the array shrinks with
// them, and three fold steps replace six or seven: 64 -> 16 as one LDS pass, 16 -> 4 and 4 -> 1 in registers
// (DPP shifts only).  Used from k = 65 up; below that the doubling arrays are faster (see the launcher).
// ------------------------------------------------------------------------------------------
template <typename OutT, int T, int TOP>
__device__ __forceinline__ void r4_fold_store(const SweepArgs &A, const Tile &t, uint32_t *lds) {
    const int LS = A.ls, HL = A.hl, m = A.nlev;
    const int cells = HL + A.w;
    // levels above 16 fold down through LDS (shifts of 16 cells and more are not a DPP's reach).  (The mixed arrays have a fold of
    // their own since round 4: plan_fold_store.)
    // Radix-4 levels: slot s holds blocks of 4^(m-1-s); after this loop slot m-3 (blocks of 16) has everything
    // above it folded in
    for (int slot = 0; slot + 3 < m; ++slot) {
        const int S = 1 << (2 * (m - 2 - slot));  // size of the blocks being folded INTO (>= 16)
        const uint32_t *hi = lds + slot * LS;
        uint32_t *lo = lds + (slot + 1) * LS;
        for (int x = 4 * threadIdx.x; x < cells; x += 4 * T) {
            uint4 r = *reinterpret_cast<const uint4 *>(lo + x);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (x >= q * S) {
                    const uint4 v = *reinterpret_cast<const uint4 *>(hi + x - q * S);
                    r.x = min(r.x, v.x);
                    r.y = min(r.y, v.y);
                    r.z = min(r.z, v.z);
                    r.w = min(r.w, v.w);
                }
            }
            *reinterpret_cast<uint4 *>(lo + x) = r;
        }
        lds_barrier();
    }
    // 16 -> 4 and 4 -> 1 in registers (memo_sweep_fold.h)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ctx = m >= 3 ? 4 : (m == 2 ? 1 : 0);  // context lanes: 15 / 3 / 0 cells to the left
    OutT *out = static_cast<OutT *>(A.out);
    const int64_t ob = t.a - A.qs - HL;  // output index of cell 0
    const int64_t o_lo = t.a - A.qs + t.x_lo, o_hi = t.a - A.qs + t.x_hi;
    fold_store_chunks<OutT, T, TOP>(out, ob, o_lo, o_hi, cells, LS, lane, wave, ctx, [&](int xr) {
        const uint32_t *p = lds + xr;
        uint4 R = *reinterpret_cast<const uint4 *>(p + (m - 1) * LS);  // blocks of 1
        if (m >= 2) {
            uint4 M = *reinterpret_cast<const uint4 *>(p + (m - 2) * LS);  // blocks of 4
            if (m >= 3) r4_fold16(M, *reinterpret_cast<const uint4 *>(p + (m - 3) * LS));
            r4_fold4(R, M);
        }
        return R;
    });
}

template <typename Rows, int U, int T, typename OutT, int TOP>
__global__ __launch_bounds__(T) __attribute__((amdgpu_waves_per_eu(8, 8)))
void sweep_conservation_r4_kernel(const SweepArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    static_assert(TOP == 0 || (!Rows::kAnnot16 && TOP == Rows::kTopShift), "the order rides in the word only in the 4-byte formats");
    const int LS = A.ls, HL = A.hl, W = A.w;
    Tile t;
    if (!locate_tile_w(A, t, W)) return;
    uint4 V[U];
    uint2 N[U];
    Rows::template issue<T, U>(A, t, 0, V, N);
    halo_clear<T>(A, lds, cell_sentinel<TOP>(A));

    const int km1 = A.km1;
    // LDS byte address of tile slot x on level i (blocks of 4^i):  level0 - i * 4 LS + 4 x
    const uint32_t ls4 = 4u * (uint32_t)LS;
    const uint32_t lds_base = (uint32_t)(size_t)(__attribute__((address_space(3))) uint32_t *)lds;
    // level i (blocks of 4^i) sits at level0 - i * 4 LS; with i' = clz(n) >> 1 = 15 - i:  levelK + i' * 4 LS
    const uint32_t levelK = pin_vgpr((int)(lds_base + (uint32_t)(A.nlev - 1) * ls4 + 4u * (uint32_t)HL - 15u * ls4));
    const uint32_t top_bit = pin_vgpr((int)0x80000000u);
    const uint32_t key = pin_vgpr((int)Rows::tile_key(t.a));
    auto scatter = [&](uint32_t w, uint32_t col) {
        // the first two blocks of a row as one branch-free block (EXEC narrowed to "n > 0" by v_cmpx, restored at the end);
        // the third and fourth stay behind the compiler's branches: where no row of a wave needs them (k = 128 on config 3)
        // skipping them beats issuing them with no lane -- 0.395 against 0.415 ms (profiles/r02_mixed_levels.txt).
        // i = floor(log4 n), S = 4^i, q = n >> 2i (the leading base-4 digit): blocks [start - n, +S) and [start - S, start);
        // q >= 2: one more at start - n + S; q = 3: and one at start - n + 2S
        uint32_t tmp, a1, a2, s4, q, dd;
        MEMO_EXEC_ALL_ONES(A.status);
#define MEMO_R4_BLOCK(LEN_SEL, REL_START)                                                                           \
        asm volatile(                                                                                               \
            "v_mov_b32 %[q], 0\n\t"                      /* q = 0 where the row does not write */                   \
            "v_sub_u32_sdwa %[n], %[km1], %[w] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD " LEN_SEL "\n\t"   \
            "v_cmpx_lt_i32 vcc, 0, %[n]\n\t"                                                                        \
            REL_START                                                                                               \
            "v_ffbh_u32 %[q], %[n]\n\t"                                                                             \
            "v_lshrrev_b32 %[q], 1, %[q]\n\t"            /* i' = 15 - i */                                          \
            "v_mad_u32_u24 %[a1], %[q], %[ls4], %[levelK]\n\t" /* level i */                                        \
            "v_lshl_add_u32 %[a2], %[rel], 2, %[a1]\n\t" /* cell `start` on level i */                              \
            "v_mad_i32_i24 %[a1], %[n], -4, %[a2]\n\t"   /* a1: cell start - n */                                   \
            "v_lshl_add_u32 %[q], %[q], 1, -1\n\t"       /* 2 i' - 1 = 29 - 2 i */                                  \
            "v_lshrrev_b32 %[s4], %[q], %[top_bit]\n\t"  /* 4 S (bytes) */                                          \
            "v_sub_u32 %[a2], %[a2], %[s4]\n\t"          /* a2: cell start - S */                                   \
            "ds_min_u32 %[a1], %[data]\n\t"                                                                         \
            "ds_min_u32 %[a2], %[data]\n\t"                                                                         \
            "v_sub_u32 %[q], 29, %[q]\n\t"               /* 2 i */                                                  \
            "v_lshrrev_b32 %[q], %[q], %[n]\n\t"         /* q */                                                    \
            "s_mov_b64 exec, -1"                                                                                    \
            : [n] "=&v"(tmp), [a1] "=&v"(a1), [a2] "=&v"(a2), [s4] "=&v"(s4), [q] "=&v"(q), [rel] "=&v"(dd)         \
            : [w] "v"(w), [km1] "s"(km1), [key] "v"(key), [ls4] "s"(ls4), [levelK] "v"(levelK),                     \
              [data] "v"(TOP ? w : col), [top_bit] "v"(top_bit)                                                     \
            : "memory", "vcc")
        if constexpr (!Rows::kW12)
            MEMO_R4_BLOCK(MEMO_ROW8_LEN_SEL, MEMO_ROW8_REL_START);
        else
            MEMO_R4_BLOCK(MEMO_ROW12_LEN_SEL, MEMO_ROW12_REL_START);
#undef MEMO_R4_BLOCK
        if (q >= 2) {
            const uint32_t data = TOP ? w : col;
            uint32_t a3, a4;
            asm volatile(
                "v_add_u32 %0, %1, %2\n\t"        // a3 = a1 + 4 S
                "ds_min_u32 %0, %3"
                : "=&v"(a3)
                : "v"(a1), "v"(s4), "v"(data)
                : "memory");
            if (q == 3) {
                asm volatile(
                    "v_add_u32 %0, %1, %2\n\t"    // a4 = a3 + 4 S
                    "ds_min_u32 %0, %3"
                    : "=&v"(a4)
                    : "v"(a3), "v"(s4), "v"(data)
                    : "memory");
            }
        }
    };
    Rows::template consume<T, U>(A, t, 0, V, N, scatter);
    for (uint32_t b = 1, nb = Rows::template batches<T, U>(t); b < nb; ++b) {  // a dense tile: the rest
        Rows::template issue<T, U>(A, t, b, V, N);
        Rows::template consume<T, U>(A, t, b, V, N, scatter);
    }
    lds_barrier();  // waits for lgkmcnt(0): the ds_min above are invisible to the compiler
    __syncthreads();
    r4_fold_store<OutT, T, TOP>(A, t, lds);
}

// ------------------------------------------------------------------------------------------
// Level plan of the mixed arrays (round 4): only the arrays some row of the index can write to are allocated, cleared and
// folded.  Which lengths n = k - 1 - overlap occur at a k follows from WHICH overlaps occur in the index -- known exactly
// since the rows were packed (memo_index::len_seen) -- and on BASELINE's generator (overlaps 0 .. 59) a k = 256 query
// has every interval in 196 .. 255: blocks of 128 only.  Six arrays (1, 4, 16, 32, 64, 128) become two (128, and the
// blocks of 16 the fold goes through), the tile grows from 1120 to 4576 positions in the same 40 KiB, and what a tile
// spends on clearing, folding and its k - 1 halo shrinks with them.  An index whose overlaps reach every level (rows
// built from sequences) gets the arrays it always got.
//   slots 0 .. D-1   the doubling RANGE: blocks of 2^(31 - ftop - d), from the largest populated size down to the
//                    smallest populated size >= 16 (a slot inside the range may be unpopulated: never cleared, never read)
//   then             the blocks of 16 when the range ends above them (the fold's target: written before it is read)
//   then             blocks of 4, blocks of 1 -- where some row can have fewer than 16 positions
// A.lvmask: bits 0..7 = populated slots of the range, kPlanSep16 / kPlanHas4 / kPlanHas1; A.nlev = D; A.ftop.
// ------------------------------------------------------------------------------------------
constexpr uint32_t kPlanSep16 = 1u << 16, kPlanHas4 = 1u << 17, kPlanHas1 = 1u << 18;

struct LevelPlan {
    int D, sep, has4, has1;
    __host__ __device__ int s16() const { return sep ? D : D - 1; }
    __host__ __device__ int s4() const { return D + sep; }
    __host__ __device__ int s1() const { return D + sep + has4; }
    __host__ __device__ int arrays() const { return D + sep + has4 + has1; }
};

__host__ __device__ inline LevelPlan plan_of(int D, uint32_t mask) {
    LevelPlan p;
    p.D = D;
    p.sep = (mask & kPlanSep16) ? 1 : 0;
    p.has4 = (mask & kPlanHas4) ? 1 : 0;
    p.has1 = (mask & kPlanHas1) ? 1 : 0;
    return p;
}

// r = min(r, the N blocks of a level at x, x - 16, ..., x - 16 (N - 1)): every read issued before the first is used (the
// loop form kept one read in flight: k = 256, fifteen reads per cell quartet, 0.55 -> 0.64 ms).  Cells left of the array do
// not exist: such a read repeats the leftmost one that does (min is idempotent), so no read is conditional.
template <int N>
__device__ __forceinline__ void fold_blocks_back(const uint32_t *hi, int x, uint4 &r) {
    const int room = x & ~15;  // the furthest multiple of 16 this lane may step back
    uint4 v[N];
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = *reinterpret_cast<const uint4 *>(hi + x - min(16 * i, room));
#pragma unroll
    for (int i = 0; i < N; ++i) {
        r.x = min(r.x, v[i].x);
        r.y = min(r.y, v[i].y);
        r.z = min(r.z, v[i].z);
        r.w = min(r.w, v[i].w);
    }
}

template <int T>
__device__ __forceinline__ void plan_clear(const SweepArgs &A, uint32_t *lds, uint32_t sent) {
    const LevelPlan P = plan_of(A.nlev, A.lvmask);
    const uint4 sv = make_uint4(sent, sent, sent, sent);
    const int per = A.ls / 4;
    // which arrays start at the sentinel: the populated slots of the range (one no row writes to is never read) and the blocks
    // of 4 / of 1; the separate target of the fold is written before it is read.  (Unrolled over the eight arrays a plan can
    // have, each behind a wave-uniform test: straight-line code the EXEC scan of tests/test_host_cpu.py can follow.)
    uint32_t wanted = A.lvmask & ((1u << P.D) - 1u);
    if (P.has4) wanted |= 1u << P.s4();
    if (P.has1) wanted |= 1u << P.s1();
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        if ((wanted >> a) & 1u) {
            uint4 *p = reinterpret_cast<uint4 *>(lds + a * A.ls);
            for (int i = threadIdx.x; i < per; i += T) p[i] = sv;
        }
    }
    lds_barrier();
}

template <typename OutT, int T, int TOP>
__device__ __forceinline__ void plan_fold_store(const SweepArgs &A, const Tile &t, uint32_t *lds) {
    const int LS = A.ls, HL = A.hl, W = A.w;
    const LevelPlan P = plan_of(A.nlev, A.lvmask);
    const int cells = HL + W;
    // every populated level above 16 into the blocks of 16, in ONE LDS pass: a block of 16 * 2^e at x covers the blocks
    // of 16 at x, x + 16, ..., x + 16 (2^e - 1)
    const int top = P.sep ? P.D - 1 : P.D - 2;  // last range slot above the blocks of 16
    if (top >= 0) {
        uint32_t *lo = lds + P.s16() * LS;
        for (int x = 4 * threadIdx.x; x < cells; x += 4 * T) {
            // (one 16-byte read whatever the plan: written as `sep ? ones : load` the compiler split it into four guarded
            // 4-byte reads -- k = 256 0.55 -> 0.64 ms; a separate target holds nothing yet, what is read there is dropped)
            uint4 r = *reinterpret_cast<const uint4 *>(lo + x);
            if (P.sep) r = make_uint4(~0u, ~0u, ~0u, ~0u);
            for (int slot = top; slot >= 0; --slot) {
                if (!((A.lvmask >> slot) & 1u)) continue;
                const uint32_t *hi = lds + slot * LS;
                switch (31 - A.ftop - slot) {  // log2 of this level's blocks (wave-uniform)
                    case 5: fold_blocks_back<2>(hi, x, r); break;
                    case 6: fold_blocks_back<4>(hi, x, r); break;
                    default: fold_blocks_back<8>(hi, x, r); break;  // blocks of 128 (k - 1 <= 255)
                }
            }
            *reinterpret_cast<uint4 *>(lo + x) = r;
        }
        lds_barrier();
    }
    // 16 -> 4 and 4 -> 1 in registers, as in r4_fold_store.  Arrays the plan does not have are read where the blocks of 16 are -- one
    // unconditional 16-byte read each -- and replaced by "no row" afterwards.
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    OutT *out = static_cast<OutT *>(A.out);
    const int64_t ob = t.a - A.qs - HL;  // output index of cell 0
    const int64_t o_lo = t.a - A.qs + t.x_lo, o_hi = t.a - A.qs + t.x_hi;
    const uint32_t *L16 = lds + P.s16() * LS, *L4 = lds + (P.has4 ? P.s4() : P.s16()) * LS,
                   *L1 = lds + (P.has1 ? P.s1() : P.s16()) * LS;
    fold_store_chunks<OutT, T, TOP>(out, ob, o_lo, o_hi, cells, LS, lane, wave, Int<4>{}, [&](int xr) {
        const uint4 ones = make_uint4(~0u, ~0u, ~0u, ~0u);
        uint4 R = *reinterpret_cast<const uint4 *>(L1 + xr);  // blocks of 1
        uint4 M = *reinterpret_cast<const uint4 *>(L4 + xr);  // blocks of 4
        if (!P.has1) R = ones;
        if (!P.has4) M = ones;
        r4_fold16(M, *reinterpret_cast<const uint4 *>(L16 + xr));
        r4_fold4(R, M);
        return R;
    });
}

// ------------------------------------------------------------------------------------------
// conservation, unclipped, MIXED levels: blocks of 1, 4, 16 and then doubling -- 32, 64, 128.
//
// What the radix-4 arrays cost is LDS atomics: an interval of n positions with 2S < n < 4S takes three or four
// blocks of S, and the sweep's time follows the blocks per row (config 3, profiles/r02_mixed_levels.txt: k = 128,
// where every interval has 64 <= n < 128 and takes two blocks, 0.39 ms; k = 101, 2.6 blocks per row, 0.515;
// k = 200, 3.5 blocks, 0.545).  At k >= 65 most intervals are long, and from 16 positions up these arrays go in
// steps of two: n >= 16 takes the two blocks of 2^floor(log2 n) of the doubling scatter, at its price (ffbh +
// five instructions after the length / validity / start triple); only n < 16 takes the radix-4 route (blocks of 4
// or of 1, two to four of them) under a branch that a wave full of long intervals never enters.  Five arrays at
// k <= 128 and six at k <= 256, where doubling alone needs seven and eight; the fold is r4_fold_store's: the
// doubling levels into the blocks of 16 in one LDS pass, 16 -> 4 -> 1 in registers.
// ------------------------------------------------------------------------------------------
template <typename Rows, int U, int T, typename OutT, int TOP>
__global__ __launch_bounds__(T) __attribute__((amdgpu_waves_per_eu(8, 8)))
void sweep_conservation_mixed_kernel(const SweepArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    static_assert(TOP == 0 || (!Rows::kAnnot16 && TOP == Rows::kTopShift), "the order rides in the word only in the 4-byte formats");
    const int LS = A.ls, HL = A.hl, W = A.w;
    const LevelPlan P = plan_of(A.nlev, A.lvmask);
    Tile t;
    if (!locate_tile_w(A, t, W)) return;
    uint4 V[U];
    uint2 N[U];
    Rows::template issue<T, U>(A, t, 0, V, N);
    plan_clear<T>(A, lds, cell_sentinel<TOP>(A));

    const int km1 = A.km1;
    // slot of the blocks of 2^(31-f), f = clz(n) <= 27:  f - ftop (the range: see the level plan above);
    // LDS byte address of tile slot x there:  bias4 + f * 4 LS + 4 x
    const uint32_t ls4 = 4u * (uint32_t)LS;
    const uint32_t lds_base = (uint32_t)(size_t)(__attribute__((address_space(3))) uint32_t *)lds;
    const uint32_t bias4 = pin_vgpr((int)(lds_base + 4u * (uint32_t)HL - (uint32_t)A.ftop * ls4));
    const uint32_t top_bit = pin_vgpr((int)0x80000000u);
    const uint32_t key = pin_vgpr((int)Rows::tile_key(t.a));
    // (rows of fewer than 16 positions exist only where the plan has arrays for them)
    uint32_t *const cells4 = lds + P.s4() * LS + HL, *const cells1 = lds + P.s1() * LS + HL;
    auto scatter = [&](uint32_t w, uint32_t col) {
        // The long intervals (n >= 16) as one branch-free block: v_cmpx narrows EXEC to "n > 0", then to "clz(n) < 28";
        // the doubling arithmetic and both ds_min run on those lanes; EXEC restored.  What is left for the
        // compiler's branch is the rare short interval (0 < n < 16).
        int n;
        uint32_t r0, r1, r2, d;
        MEMO_EXEC_ALL_ONES(A.status);
#define MEMO_MIXED_BLOCK(LEN_SEL, REL_START)                                                                        \
        asm volatile(                                                                                               \
            "v_sub_u32_sdwa %[n], %[km1], %[w] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD " LEN_SEL "\n\t"   \
            REL_START                                                                                               \
            "v_ffbh_u32 %[f], %[n]\n\t"                                                                             \
            "v_cmpx_lt_i32 vcc, 0, %[n]\n\t"                                                                        \
            "v_cmpx_gt_u32 vcc, 28, %[f]\n\t"                                                                       \
            "v_mad_u32_u24 %[a2], %[f], %[ls4], %[bias4]\n\t"                                                       \
            "v_lshl_add_u32 %[a2], %[rel], 2, %[a2]\n\t"                                                            \
            "v_mad_i32_i24 %[a1], %[n], -4, %[a2]\n\t"                                                              \
            "v_ashrrev_i32 %[f], %[f], %[top_bit]\n\t"                                                              \
            "v_lshl_add_u32 %[a2], %[f], 2, %[a2]\n\t"                                                              \
            "ds_min_u32 %[a1], %[data]\n\t"                                                                         \
            "ds_min_u32 %[a2], %[data]\n\t"                                                                         \
            "s_mov_b64 exec, -1"                                                                                    \
            : [f] "=&v"(r0), [a1] "=&v"(r1), [a2] "=&v"(r2), [n] "=&v"(n), [rel] "=&v"(d)                           \
            : [w] "v"(w), [km1] "s"(km1), [key] "v"(key), [ls4] "s"(ls4), [bias4] "v"(bias4), [top_bit] "v"(top_bit), \
              [data] "v"(TOP ? w : col)                                                                             \
            : "memory", "vcc")
        if constexpr (!Rows::kW12)
            MEMO_MIXED_BLOCK(MEMO_ROW8_LEN_SEL, MEMO_ROW8_REL_START);
        else
            MEMO_MIXED_BLOCK(MEMO_ROW12_LEN_SEL, MEMO_ROW12_REL_START);
#undef MEMO_MIXED_BLOCK
        if ((uint32_t)(n - 1) < 15u) {  // 0 < n < 16: blocks of S = 4 (n >= 4) or 1 at start - n and start - S; two more while n >= 2S, 3S
            const uint32_t data = TOP ? w : col;
            const bool four = n >= 4;
            uint32_t *lv = (four ? cells4 : cells1) + d;
            const int S = four ? 4 : 1, q = four ? n >> 2 : n;
            atomicMin(lv - n, data);
            atomicMin(lv - S, data);
            if (q >= 2) atomicMin(lv - n + S, data);
            if (q == 3) atomicMin(lv - n + 2 * S, data);
        }
    };
    Rows::template consume<T, U>(A, t, 0, V, N, scatter);
    for (uint32_t b = 1, nb = Rows::template batches<T, U>(t); b < nb; ++b) {  // a dense tile: the rest
        Rows::template issue<T, U>(A, t, b, V, N);
        Rows::template consume<T, U>(A, t, b, V, N, scatter);
    }
    lds_barrier();  // waits for lgkmcnt(0): the ds_min above are invisible to the compiler
    __syncthreads();
    plan_fold_store<OutT, T, TOP>(A, t, lds);
}

// k <= 1: no row can write (casted_end >= start always), every position keeps its initial value
template <typename OutT>
__global__ void fill_conservation_kernel(OutT *out, int64_t n, OutT v) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        out[i] = v;
}

// One workgroup per row with end < start: its interval [clip(e-qs-(k-1)), clip(s-qs)) can be any
// length, so it is applied straight to the result in HBM, after the sweep, with atomics (rows may
// overlap each other).  filter_pq keeps such a row iff qs < start < qe + k (memo_query.py:25-27).
// The result has no 8- or 16-bit atomics, so a value is min-ed by a CAS on its 32-bit word; the word
// that holds the last L % (4 / sizeof(OutT)) values would reach past the caller's buffer, so those
// (at most 3) positions are left to long_rows_tail_kernel.
template <typename OutT>
__device__ __forceinline__ bool long_row_interval(int64_t s, int64_t e, int64_t o, int64_t qs, int64_t qe, int km1,
                                                  int ncols, int *status, int64_t &c, int64_t &hi, int64_t &cc,
                                                  int64_t fqs, int64_t fqe) {
    // [fqs, fqe) = the window the reference's filter sees (= [qs, qe) unless this sweep is a sub-window of it)
    if (!(s > fqs && s < fqe + km1 + 1)) return false;
    const int64_t L = qe - qs;
    hi = s - qs > L ? L : s - qs;
    c = e - qs - km1;
    c = c < 0 ? 0 : c;
    if (c >= hi) return false;
    cc = o < 0 ? o + ncols : o;
    if ((uint64_t)cc >= (uint64_t)ncols) {
        if (threadIdx.x == 0) atomicOr(status, kStatusBadAnnot);
        return false;
    }
    return true;
}

template <typename OutT>
__global__ void long_rows_conservation_kernel(const int64_t *ls, const int64_t *le, const int64_t *lo,
                                              int64_t qs, int64_t qe, int km1, int ncols, OutT *out,
                                              int *status, int64_t fqs, int64_t fqe) {
    int64_t c, hi, cc;
    if (!long_row_interval<OutT>(ls[blockIdx.x], le[blockIdx.x], lo[blockIdx.x], qs, qe, km1, ncols, status, c, hi, cc,
                                 fqs, fqe))
        return;
    constexpr int PER = 4 / (int)sizeof(OutT);  // results per 32-bit word
    const int64_t whole = (qe - qs) / PER * PER;  // positions whose word lies inside the buffer
    if (hi > whole) hi = whole;
    uint32_t *words = reinterpret_cast<uint32_t *>(out);
    for (int64_t p = c + threadIdx.x; p < hi; p += blockDim.x) {
        uint32_t *wp = words + p / PER;
        const int sh = (int)(p % PER) * 8 * (int)sizeof(OutT);
        const uint32_t field = (sizeof(OutT) == 2 ? 0xFFFFu : 0xFFu) << sh;
        uint32_t old = *wp;
        while (((old & field) >> sh) > (uint32_t)cc) {  // out[p] = min(out[p], col), on the field only
            const uint32_t seen = atomicCAS(wp, old, (old & ~field) | ((uint32_t)cc << sh));
            if (seen == old) break;
            old = seen;
        }
    }
}

// the last L % PER positions: one workgroup reduces, per position, the smallest column over ALL rows
// with end < start and stores it with a plain element store (nothing else writes there any more)
template <typename OutT>
__global__ __launch_bounds__(256) void long_rows_tail_kernel(const int64_t *ls, const int64_t *le, const int64_t *lo,
                                                             uint64_t n_long, int64_t qs, int64_t qe, int km1,
                                                             int ncols, OutT *out, int *status, int64_t fqs,
                                                             int64_t fqe) {
    constexpr int PER = 4 / (int)sizeof(OutT);
    const int64_t L = qe - qs, whole = L / PER * PER;
    __shared__ uint32_t best[4];
    if (threadIdx.x < 4) best[threadIdx.x] = 0xFFFFFFFFu;
    __syncthreads();
    for (uint64_t r = threadIdx.x; r < n_long; r += 256) {
        int64_t c, hi, cc;
        // (the bad-annot flag is raised by thread 0 of the main kernel's workgroup for this row)
        const int64_t s = ls[r], e = le[r], o = lo[r];
        if (!(s > fqs && s < fqe + km1 + 1)) continue;
        hi = s - qs > L ? L : s - qs;
        c = e - qs - km1;
        c = c < 0 ? 0 : c;
        cc = o < 0 ? o + ncols : o;
        if (c >= hi || (uint64_t)cc >= (uint64_t)ncols) continue;
        for (int64_t p = whole > c ? whole : c; p < hi; ++p) atomicMin(&best[p - whole], (uint32_t)cc);
    }
    __syncthreads();
    if (threadIdx.x < L - whole && best[threadIdx.x] < (uint32_t)out[whole + threadIdx.x])
        out[whole + threadIdx.x] = (OutT)best[threadIdx.x];
}

}  // namespace

constexpr int kHaloLoads = 6;  // 16-byte loads in flight per lane

template <typename OutT>
static int long_rows_conservation(const memo_index *ix, int64_t qs, int64_t qe, int32_t k, int ncols,
                                  OutT *d_out, hipStream_t st) {
    if (!ix->long_rows.n || g_prepare_only) return MEMO_OK;
    if (int prc = refuse_plan_pointer(d_out)) return prc;
    const int64_t fqs = ix->whole_set ? ix->whole_qs : qs, fqe = ix->whole_set ? ix->whole_qe : qe;
    hipLaunchKernelGGL((long_rows_conservation_kernel<OutT>), dim3((unsigned)ix->long_rows.n), dim3(256), 0, st,
                       ix->long_rows.s(), ix->long_rows.e(), ix->long_rows.o(), qs, qe, k - 1, ncols, d_out, ix->d_status, fqs, fqe);
    if ((qe - qs) % (4 / (int)sizeof(OutT)))
        hipLaunchKernelGGL((long_rows_tail_kernel<OutT>), dim3(1), dim3(256), 0, st, ix->long_rows.s(), ix->long_rows.e(), ix->long_rows.o(),
                           (uint64_t)ix->long_rows.n, qs, qe, k - 1, ncols, d_out, ix->d_status, fqs, fqe);
    HIP_TRY(hipGetLastError());
    return MEMO_OK;
}

// Which level arrays for the unclipped sweep at k - 1 >= 64: 2 = doubling, 3 = radix-4, 4 = mixed.
// What separates them is LDS atomics per row against level arrays per tile (profiles/r02_mixed_levels.txt, config 3):
// every row costs two blocks on doubling and mixed arrays (mixed: when its interval has 16 positions or more), two
// to four on radix-4 arrays -- 0.39 ms at two blocks per row, +0.14 ms per extra block -- and every array beyond
// four costs clear, fold and tile length: five arrays +0.03 ms, six +0.1, doubling's seven or eight +0.17 / +0.25.
// The interval lengths n = k - 1 - overlap are known in distribution from the overlaps sampled when the packed rows
// were made (memo_index.len_hist), so: many intervals under 16 positions (mixed would keep entering its slow path)
// -> doubling up to seven levels (k <= 128; its fold runs in registers) and on dense indexes, else radix-4; radix-4
// within 0.15 blocks per row of two (0.9 where mixed needs six arrays) -> radix-4; else mixed.
// The level plan of the mixed arrays for k - 1 = km1 (see plan_of above): returns D, the slots of the doubling range; *ftop =
// clz of the range's largest block size; *mask = populated slots | kPlanSep16 | kPlanHas4 | kPlanHas1.  `all`: every array a
// k - 1 of this size can need (rounds 2-3; also what an index without an exact census gets).
static int level_plan(const memo_index *ix, int km1, bool all, int *ftop, uint32_t *mask) {
    all = all || !ix->len_seen_exact;
    bool lv[32] = {false};
    bool has4 = false, has1 = false;
    for (int len = 0; len < km1 && len < 256; ++len) {
        if (!all && !((ix->len_seen[len >> 5] >> (len & 31)) & 1u)) continue;  // no row of the index has this overlap
        const int n = km1 - len;
        if (n >= 16) lv[__builtin_clz((unsigned)n)] = true;
        else if (n >= 4) has4 = true;
        else has1 = true;
    }
    int top = 32, bot = -1;
    for (int f = 0; f <= 27; ++f)
        if (lv[f]) {
            top = f < top ? f : top;
            bot = f;
        }
    if (bot < 0) top = bot = 27, lv[27] = true;  // (no row of 16 positions or more: the blocks of 16 alone, which nobody writes)
    uint32_t m = 0;
    for (int f = top; f <= bot; ++f)
        if (lv[f]) m |= 1u << (f - top);
    if (bot < 27) m |= kPlanSep16;
    if (has4) m |= kPlanHas4;
    if (has1) m |= kPlanHas1;
    *ftop = top;
    *mask = m;
    return bot - top + 1;
}

static int pick_levels(const memo_index *ix, int k, bool moderate) {
    const int km1 = k - 1, fallback = (km1 < 128 || !moderate) ? 2 : 3;
    if (!ix->len_hist_rows) return fallback;
    double rows = 0, blocks4 = 0, small = 0;
    for (int len = 0; len < 256 && len < km1; ++len) {
        const double w = ix->len_hist[len];
        const int n = km1 - len;
        const int i = floor_log2((uint32_t)n) >> 1, q = n >> (2 * i);  // radix-4: blocks of 4^i, leading digit q
        rows += w;
        blocks4 += w * (q == 1 ? 2 : q + 1);
        if (n < 16) small += w;
    }
    if (rows <= 0) return fallback;
    // What decides (profiles/r04_large_k.txt): level arrays per tile against blocks per row -- and on an index of moderate density
    // the arrays weigh more (rows built from sequences, 2 x 20 Mbp x 50 genomes, one more array costs what 0.3 blocks per row
    // cost).  The mixed arrays take two blocks per row and exist only where some row can write (level_plan): with no more of them
    // than radix-4's four they are the choice (BASELINE's generator at every k >= 65: two or three arrays).  Where the overlaps
    // reach every level (rows built from sequences: five or six mixed arrays, seven or eight doubling ones) radix-4 arrays win
    // while a row takes few blocks -- k = 101: 2.3 blocks per row, 0.185 ms against 0.204 doubling and 0.208 mixed; k = 128: 0.198
    // against 0.228; k = 160: 0.248 against 0.272 mixed -- and lose beyond ~2.9 (k = 65: 0.181 against 0.168 doubling; k = 200:
    // 0.284 against 0.279 mixed).  Many intervals under 16 positions keep the mixed arrays out (their slow path).
    const bool few_small = small <= 0.03 * rows;
    int ftop = 0;
    uint32_t mask = 0;
    const int planned = ix->len_seen_exact ? plan_of(level_plan(ix, km1, false, &ftop, &mask), mask).arrays() : 99;
    if (few_small && planned <= 4) return 4;
    if (moderate && blocks4 <= 2.9 * rows) return 3;
    if (few_small) return ix->len_seen_exact || blocks4 > (km1 >= 128 && moderate ? 2.9 : 2.15) * rows ? 4 : 3;
    return fallback;
}

// Tile of the clipped sweep: the debug tile width as a power of two up to 4096, else the widest tile whose doubling arrays fit
// the budget, narrowed on short windows.
static int clipped_width(int tile_w, int nlev, size_t budget, int64_t len) {
    int w = tile_w;
    while (w & (w - 1)) w &= w - 1;  // (the clipped kernels and the doubling arrays come in powers of two)
    if (w > 4096) w = 4096;
    if (!w) {
        w = 4096;
        while ((size_t)nlev * w * 4 > budget && w > 256) w >>= 1;
        while (w > 1024 && len / w < 8192) w >>= 1;                // big 4-wave tiles: a few thousand suffice
        while (w > 256 && w <= 1024 && len / w < 32768) w >>= 1;  // short windows: many small tiles
    }
    return w;
}

// Tile of the radix-4 and mixed level arrays: m arrays of ls cells (the debug tile width, else ls0), halo hl left and hr right
// of a tile of tw positions (whole buckets).  fits: the tile holds a bucket, the halo is at most two thirds, the arrays fit in LDS.
struct LevelTile {
    int hl, hr, ls, tw;
    bool fits;
};
static LevelTile level_tile(int bw, int km1, int fmt, int64_t len, int tile_w, int ls0, int m) {
    LevelTile t;
    t.hl = (km1 + 3) & ~3;
    t.hr = (km1 + bw - 1 + 3) & ~3;
    int ls = tile_w ? tile_w : ls0;
    if (ls > 8192) ls = 8192;
    if (fmt == 12 && ls > 4096) ls = 4096;  // (12-bit start field: start - a < array size <= 2^12)
    // short windows: enough tiles to fill the chip (a few thousand of them)
    while (!tile_w && ls > 640 && len / (ls - t.hl - t.hr > bw ? ls - t.hl - t.hr : bw) < 4096) ls = (ls / 2) & ~3;
    t.ls = ls;
    t.tw = (ls - t.hl - t.hr) / bw * bw;
    t.fits = t.tw >= bw && 2 * t.tw >= t.hl + t.hr && (size_t)m * (t.hl + t.tw + t.hr) * 4 <= 160 * 1024;
    return t;
}

// The dense rows of this k's class (a view that leaves out the rows that cannot write at this k), or all of them, for the
// unclipped doubling tile in A.  Views of six rows per group are for the table-driven kernel alone: a query it cannot take (a
// negative window start, no room for the tile table) asks again for five-row groups.  The table-driven kernel sweeps the dense
// rows wherever the query fits it; only the debug row sources 5 and 10 (tune.persistent == 1) keep them on
// sweep_conservation_halo3_kernel.  *variant: 2 / 3 when the table-driven kernel answered on five- / six-row groups, 4 when the run copy
// of this k - 1 was decoded in the sweep's place; 0: A holds
// five-row groups for sweep_conservation_halo3_kernel.
static int sweep_dense_rows(memo_index *ix, SweepArgs &A, int tw, int elem_bytes, bool top8, bool top9, hipStream_t st,
                            int *variant) {
    const memo_tuning &tune = ix->tune;
    const bool table = tune.persistent == 5 || tune.persistent == 0;
    *variant = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        const bool can_six = attempt == 0 && table && top8 && A.nlev <= 5 && A.qs >= 0;
        RowSource src;  // (memo_view.h; rpg 6: a view whose groups carry their bucket)
        if (int rc = dense_rows_for(ix, A.km1, A.qe - A.qs, st, src, can_six, attempt == 0)) return rc;
        A.p3 = src.p3;
        A.boff = src.boff;
        note_dense_rows_read(ix, src);
        if (src.run_tab) {  // the run copy of this k - 1 answers: results are decoded, no row is swept (memo_sweep_runs.hip)
            if (int rc = launch_runs_decode(ix, A, src, elem_bytes, st)) return rc;
            *variant = 4;
            return MEMO_OK;
        }
        if (table) {
            // the tile's row slice from a table built once per (index, k): memo_sweep_cons3t.hip; 1 = does not fit
            // (a view whose cap is k - 1 holds exactly the rows that write at this k: the table-driven kernel's row blocks drop their test)
            const int trc = launch_halo3t(ix, A, tw, elem_bytes, st, top9, src.cap == A.km1 && !tune.no_all_write, src.rpg == 6,
                                          src.rpg == 6 && src.placed && src.dead_share >= kLiveMinShare);
            if (trc < 0) return trc;
            if (trc == MEMO_OK) {
                *variant = src.rpg == 6 ? 3 : 2;
                return MEMO_OK;
            }
        }
        if (src.rpg != 6) return MEMO_OK;  // (five-row groups: the kernel without a table takes them)
    }
    return fail(MEMO_EHIP, "a six-row view reached a sweep that cannot read it");
}

template <typename OutT>
static int query_conservation(memo_index_t *ix, int64_t qs, int64_t qe, int32_t k, int32_t num_docs,
                              OutT *d_out, void *stream) {
    int rc = check_query_args(ix, qs, qe, k, num_docs, d_out);
    if (rc) return rc;
    if (sizeof(OutT) == 1 && num_docs > 255)
        return fail(MEMO_EINVAL, "uint8 results need num_docs <= 255, got %d", num_docs);
    if (qe <= qs) return MEMO_OK;
    DeviceGuard guard(ix->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (k <= 1 || ix->rows == 0) {
        if (g_prepare_only) return MEMO_OK;
        if ((rc = refuse_plan_pointer(d_out))) return rc;
        ix->last_pick = memo_index::SweepPick();  // (no sweep: the fill)
        hipLaunchKernelGGL((fill_conservation_kernel<OutT>), dim3(2048), dim3(256), 0, st, d_out,
                           qe - qs, (OutT)num_docs);
        HIP_TRY(hipGetLastError());
        return long_rows_conservation<OutT>(ix, qs, qe, k, num_docs + 1, d_out, st);
    }
    SweepArgs A;
    fill_args(ix, A, qs, qe, k, d_out);
    A.ncols = num_docs + 1;
    A.nlev = floor_log2((uint32_t)(k - 1)) + 1;
    A.nwords = 0;
    int fmt;
    if ((rc = pick_rows(ix, k, fmt))) return rc;

    // -- the plan: the kernel family (numbered as memo_index_info_t.last_sweep: 1 clipped, 2 doubling, 3 radix-4, 4 mixed,
    //    5 the dense rows), its kernel and its tile
    const memo_tuning &tune = ix->tune;
    const int km1 = k - 1, bw = 1 << ix->bshift;
    const int64_t len = qe - qs;
    // Tile shape, from interleaved A/B on one device (profiles/r01_ab_*.txt).
    //  int64 rows (HBM-bound): four waves share a 4096-position tile -- fewest k-1 row halos per
    //    position; 1-3 % over one wave per 1024 positions at k <= 32, 10 % at k = 101.
    //  packed rows (4-6x fewer bytes; LDS-atomic / issue-bound): waves per CU matter, but so does
    //    the k-1 halo: 1024 positions x 4 waves wins at k = 31 (20 KiB, 8 workgroups per CU) and at
    //    k = 101 (28 KiB) over 512 or 2048 positions.
    // Short windows want many small tiles either way.
    // int64 rows on a sparse index (< 2 rows per position: profiles/r01_sparse_index_tiles.txt) are
    // no longer HBM-bound per tile; they want the packed rows' shape (more workgroups per CU)
    const double span = (double)(ix->max_s - ix->min_s) + 1.0;
    const bool sparse = (double)ix->rows < 2.0 * span;
    auto clipped_budget = [&] { return (fmt || sparse) ? (size_t)32 * 1024 : (size_t)80 * 1024; };
    auto clipped_waves = [&](int ww) { return tune.waves == 1 || tune.waves == 4 ? tune.waves : (ww >= 1024 ? 4 : 1); };
    int w = clipped_width(tune.tile_w, A.nlev, clipped_budget(), len);
    int waves = clipped_waves(w);  // short windows end up with small tiles: one wave each
    const bool checked = ix->max_annot >= (uint64_t)A.ncols;  // some row could be outside the matrix
    // unclipped scatter (PackedRows, every annot inside the matrix): w is the size of a level array,
    // HL + tile + HR cells (start - a <= tile + k + 30 inside a slice); the tile is what is left
    // after the halo, rounded down to whole buckets
    // (below one row per position the halo's extra clear and fold cost more than the scatter saves)
    bool halo = fmt && !checked && (tune.scatter >= 2 || (tune.scatter == 0 && (double)ix->rows >= span));
    // Radix-4 levels (sweep_conservation_r4_kernel) from k = 65 up on indexes of moderate density: four arrays
    // where doubling needs seven or eight.  Interleaved A/B (profiles/r02_radix4_levels.txt; doubling -> radix-4,
    // ms): config 3 (5 rows per position) k = 101 0.564 -> 0.514, k = 256 0.951 -> 0.668, with arrays of 2560
    // cells shared by eight waves (40 KiB, four workgroups per CU).  At k = 21 / 31 / 64 the doubling arrays stay
    // ahead (0.375 vs 0.40, 0.46 vs 0.50), and so they do at any k on a dense index -- config 5, 25 rows per
    // position: k = 101 0.89 vs 1.08, k = 256 1.14 vs 1.55 -- where a row's third and fourth block cost more LDS
    // atomics than the fold steps save.
    const bool moderate = (double)ix->rows < 12.0 * span;
    // (debug switch scatter = 5: the mixed arrays with the library's level plan, whatever pick_levels would say)
    const int levels = !halo || fmt == 3 ? 0 : tune.scatter == 5 ? 4 : tune.scatter >= 2 ? tune.scatter : (km1 >= 64 ? pick_levels(ix, k, moderate) : 2);
    SweepKernel kern = nullptr;
    int sweep = 0, tw = 0, arrays = 0;
    size_t lds = 0;
    bool three = false, top9 = false, top8 = false, doubling_tile = false;
    memo_index::SweepPick pick;  // what the pickers below were handed (memo_index::last_pick; launch_halo3t adds the table-driven sweep's)
    pick.out_bytes = (int32_t)sizeof(OutT);
    // Mixed levels (sweep_conservation_mixed_kernel): 1, 4, 16, then doubling -- of which only the arrays some row of the index
    // can write to exist (level_plan; the debug switch scatter = 4 asks for all of them, the layout of rounds 2-3).  k - 1 >= 16.
    if (levels == 3 || (levels == 4 && km1 >= 16)) {
        int ftop = 0, m = 0, D = 0;
        uint32_t mask = 0;
        if (levels == 3) {
            D = m = (floor_log2((uint32_t)km1) >> 1) + 1;
        } else {
            D = level_plan(ix, km1, tune.scatter == 4, &ftop, &mask);
            m = plan_of(D, mask).arrays();
        }
        const LevelTile t = level_tile(bw, km1, fmt, len, tune.tile_w, levels == 3 ? 2560 : (40 * 1024 / (4 * m)) & ~63, m);
        if (t.fits) {
            A.nlev = D;
            A.lvmask = mask;
            A.ftop = ftop;
            A.hl = t.hl;
            A.w = tw = t.tw;
            A.ls = t.hl + t.tw + t.hr;
            waves = tune.waves == 1 || tune.waves == 4 || tune.waves == 8 ? tune.waves : (t.ls >= (levels == 3 ? 2048 : 1536) ? 8 : 4);
            sweep = levels;
            arrays = m;
            lds = (size_t)m * A.ls * 4;
            kern = pick_packed<false>(fmt, [&](auto R) {
                using Rows = typename decltype(R)::type;
                return pick_top<Rows>(num_docs, [&](auto TOP) {
                    return pick_int<512, 256, 64>(threads_of(waves), [&](auto T) {
                        pick.top = TOP, pick.threads = T;
                        return levels == 3 ? (SweepKernel)sweep_conservation_r4_kernel<Rows, kHaloLoads, T, OutT, TOP>
                                           : (SweepKernel)sweep_conservation_mixed_kernel<Rows, kHaloLoads, T, OutT, TOP>;
                    });
                });
            });
        }
    }
    if (!kern && halo) {
        // A/B (profiles/r01_unclipped_scatter.txt): arrays of 1024 cells x 4 waves win at every window
        // length from 10^6 positions up and at k = 21 .. 101
        // (a slice ends at a bucket boundary: start - a <= tile + k - 1 + bw - 2)
        const int hl = (km1 + 3) & ~3, hr = (km1 + bw - 1 + 3) & ~3;
        if (!tune.tile_w) w = km1 >= 128 ? 2048 : 1024;  // (k = 256 on config 5: 1.40 ms with 1024 cells x 4 waves, 1.14 with 2048 x 8)
        for (;; w <<= 1) {
            tw = (w - hl - hr) / bw * bw;
            if ((tw >= bw && 2 * tw >= hl + hr) || w >= 4096) break;  // keep the halo under two thirds of the array
        }
        while ((size_t)A.nlev * (hl + tw + hr) * 4 > 160 * 1024 && tw > bw) tw = (tw / 2 + bw - 1) / bw * bw;
        if (tw < bw) halo = false;
        else {
            doubling_tile = true;
            A.hl = hl;
            A.w = tw;
            A.ls = hl + tw + hr;
            if (tune.waves == 0) waves = w >= 2048 ? 8 : (w >= 1024 ? 4 : 1);
            if (tune.waves == 8) waves = 8;
            // The dense rows where they are resident and can answer (k - 1 <= 63, level arrays within 2^10 cells,
            // num_docs <= 255): a fifth fewer bytes for three more instructions per row.  Back to back -- thousands
            // of launches, the device settled at its power cap (1345-1375 W of 1400) -- they are 13 % faster at
            // k = 21 / 31 and 4-7 % at k = 48 / 64 (config 3: 0.324 against 0.374 ms on one device;
            // profiles/r02_dense_rows_ab.txt).  Short interleaved timings had shown them level: a switch of kernels
            // sets off a swing of the clocks that lasts some thirty launches, and the dense kernel, which draws more
            // power per unit of time, sits on the cap at a lower clock (2.2 against 2.36 GHz).
            top8 = num_docs <= 255;
            // (the dense rows may leave out the rows that can never write at k <= 64 -- memo_common.h: boff3 -- and then have
            // their own row numbers and bucket table; they answer only while they still hold a row per position)
            const uint64_t drows = ix->boff3 ? ix->rows3 : ix->rows;
            // 256 .. 511 genomes: the table-driven kernel's nine-bit form (memo_sweep_cons3t.hip: A9), uint16 results, or not the dense rows
            top9 = !top8 && num_docs <= 511 && ix->max_annot <= 511 && sizeof(OutT) == 2;
            three = ix->p3 && (!ix->pk || !tune.force_packed) && km1 <= 63 && A.ls <= 1024 && (top8 || top9) &&
                    ((double)drows >= span || !ix->pk);
            if (three || fmt != 3) {  // (else the int64 columns below, or an error when they are gone too)
                sweep = three ? 5 : 2;
                lds = (size_t)A.nlev * A.ls * 4;
                kern = pick_int<512, 256, 64>(threads_of(waves), [&](auto T) -> SweepKernel {
                    pick.threads = T;
                    if (three) {  // (no tile table: no room, a negative window start)
                        if constexpr (sizeof(OutT) == 2) {
                            if (top9)  // (256 .. 511 genomes)
                                return (SweepKernel)sweep_conservation_halo3_kernel<PackedRows3::kLoads, T, OutT, true>;
                        }
                        return (SweepKernel)sweep_conservation_halo3_kernel<PackedRows3::kLoads, T, OutT>;
                    }
                    return pick_packed<false>(fmt, [&](auto R) {
                        using Rows = typename decltype(R)::type;
                        return pick_top<Rows>(num_docs, [&](auto TOP) {
                            pick.top = TOP;
                            return (SweepKernel)sweep_conservation_halo_kernel<Rows, kHaloLoads, T, OutT, TOP>;
                        });
                    });
                });
            } else {
                halo = false;
            }
        }
    }
    if (!halo) {  // the clipped sweep (w: 4096 when no doubling tile fits)
        if (fmt == 3) {  // the dense rows cannot answer this one (tile shape, num_docs > 255, sparse index)
            if (!ix->has_wide)
                return fail(MEMO_EINVAL, "this query needs the 4-byte rows or the int64 columns, which this index dropped");
            fmt = 0;
            w = clipped_width(tune.tile_w, A.nlev, clipped_budget(), len);  // tile shape for int64 rows
            waves = clipped_waves(w);
        }
        if (fmt == 12 && w > 2048) w = 2048;  // a 12-bit start field: the slice of a tile spans less than 2^12 positions
        while ((size_t)A.nlev * w * 4 > 160 * 1024 && w > 256) w >>= 1;
        A.hl = 0;
        A.w = tw = w;
        A.ls = w;
        sweep = 1;
        lds = (size_t)A.nlev * A.ls * 4;
        kern = pick_rows_clipped(fmt, checked, [&](auto R) {
            using Rows = typename decltype(R)::type;
            return pick_int<256, 512, 1024, 2048, 4096>(w, [&](auto W) {
                return pick_int<256, 64>(clipped_threads_of(waves), [&](auto T) {
                    pick.threads = T, pick.width = W;
                    return (SweepKernel)sweep_conservation_kernel<Rows, W, Rows::kLoads, T, OutT>;
                });
            });
        });
        if (!kern) return fail(MEMO_EINVAL, "unsupported tile width %d", w);
    }

    // -- the rows, the launch, the record
    int variant = 0;
    if (doubling_tile) ix->last_variant = ix->last_tile_w = 0;
    ix->last_tiles_per_group = 1;  // (launch_halo3t says otherwise)
    pick.family = sweep;
    pick.format = three ? 3 : fmt;
    pick.checked = sweep == 1 && fmt && checked;  // (pick_rows_clipped; every other family is handed CHECKED = false)
    if (sweep != 1) pick.width = A.ls;
    pick.arrays = sweep == 3 || sweep == 4 ? arrays : A.nlev;
    pick.a9 = three && top9;
    ix->last_pick = pick;
    if (three) {
        if ((rc = sweep_dense_rows(ix, A, tw, (int)sizeof(OutT), top8, top9, st, &variant))) return rc;
    } else if ((rc = use_words(ix, A, fmt, false, st))) {
        return rc;
    }
    if (!variant && (rc = launch_tiles(kern, A, tw, 64 * waves, lds, st))) return rc;
    if (three && !variant) ix->last_pick.halo3 = 1;
    ix->last_sweep = sweep;
    if (sweep == 4) ix->last_arrays = arrays;
    if (variant) ix->last_variant = variant;
    return long_rows_conservation<OutT>(ix, qs, qe, k, A.ncols, d_out, st);
}

extern "C" {

int memo_query_conservation_dev(memo_index_t *ix, int64_t qs, int64_t qe, int32_t k,
                                int32_t num_docs, uint16_t *d_out, void *stream) {
    return query_conservation<uint16_t>(ix, qs, qe, k, num_docs, d_out, stream);
}

int memo_query_conservation_u8_dev(memo_index_t *ix, int64_t qs, int64_t qe, int32_t k,
                                   int32_t num_docs, uint8_t *d_out, void *stream) {
    return query_conservation<uint8_t>(ix, qs, qe, k, num_docs, d_out, stream);
}

}  // extern "C"
