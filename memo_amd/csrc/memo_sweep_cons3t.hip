// memo_sweep_cons3t.hip -- the conservation sweep on the dense rows, one workgroup per tile, with the tile's row slice
// read from a TILE TABLE instead of being worked out by every wave (round 3; the counterpart of
// /root/reference/src/memo_query.py:42-63 + :70 like every sweep here).
//
// sweep_conservation_halo3_kernel (memo_sweep_cons.hip) spends ~300 scalar instructions per wave, ~130 of them finding
// its tile: 64-bit tile arithmetic, two divisions by five, two dependent bucket-table loads, bounds.  The CU has one
// scalar unit, and the sweep's time follows its scalar instruction count (+100 do-nothing SALU per wave: +6.6 %; +100
// VALU: +5.3 %; profiles/r03_issue_diagnostic.txt).  A tile's slice -- first group, groups, first and last valid row --
// depends on the index, the tile width and k only (tiles are aligned in PIVOT coordinates), so it is computed once per
// (index, k) by tile_table_kernel, 32 bytes per tile (3.4 MB for BASELINE config 3), kept with the index, and every
// later query's waves fetch their tile with ONE s_load_dwordx8.  The rest of the tile body is the lean one of
// memo_sweep_dense.h: clear, level reads and fold unrolled for the number of level arrays (template parameter), four
// row loads in a row, rows masked by number only in the pieces that straddle an end of the slice.
//
// The wide tiles (R4) run a kernel of their own, sweep_conservation_wide_kernel, whose time follows the chain a tile walks while it
// holds its 20 KiB, not its instruction count.  Three links of that chain are gone (profiles/tile_chain.txt: -6.7 ... -7.1 % at
// k = 31, 21, 17, each part alone faster than the kernel before on every run):
//   - the head: the six values a wave needs before its row loads, and six more it needs before the barrier, are leading scalar
//     kernel parameters, which gfx950 delivers in SGPRs at wave launch (kernel-argument preload, 14 dwords; this file is compiled
//     with -amdgpu-kernarg-preload-count=16); the tile descriptor then comes with ONE s_load_dwordx8 -- one scalar round trip in
//     front of the row loads where there were several;
//   - the fold: a wave with two chunks of the level arrays reads both before it waits (fold_chunks_once_or_twice);
//   - the store: a tile that touches neither edge of the window keeps the lanes right of the left halo and stores their four
//     results at a scalar base plus a 32-bit lane offset; the per-cell 64-bit window test is left to the window's first and last
//     tile.  The wave-uniform choice is made once, in front of two straight tails (made per store it cost what it saved).
// memo_debug_set_tuning (scatter bits 8 .. 10) switches each part off; all off is sweep_conservation_halo3t_kernel<..., R4>.
// Where the wide tiles hold few groups a workgroup sweeps TWO of them behind one head (sweep_conservation_wide_pair_kernel,
// profiles/tile_pairs.txt; scatter bit 11 switches that off).
#include "memo_sweep_dense.h"

using namespace memo;
using namespace memo::dense;

namespace {

struct TileDesc {  // 32 bytes
    uint32_t g0_lo, g0_hi;  // first group of the slice (five-row groups: a multiple of 8)
    uint32_t ng;            // groups; 0xFFFFFFFF: more than 2^32 rows reach this tile (unsupported)
    uint32_t first, end;    // rows [first, end) of the slice, counted from row 5 * g0
    uint32_t g_wrap;        // six-row groups: the first group of the slice (counted from g0) whose bucket lies 1024 or more positions past
                            // the tile's first one (a group carries its bucket mod 32; the R4 kernel's wide tiles reach past 1024 cells)
    uint32_t pad[2];
};

// tile T covers pivot positions [T * w, (T + 1) * w); its rows: T * w <= start < roundup((T + 1) * w + k - 1, bucket)
// rpg: rows per group -- 5, or 6 (A/B: groups that carry their bucket)
__global__ void tile_table_kernel(const int64_t *boff, int64_t nb, int64_t bbase, int bshift, int w, int km1, int64_t ntab,
                                  TileDesc *out, int rpg) {
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t >= ntab) return;
    const int64_t a = t * w, last = nb - 1, lim = a + w + km1;
    int64_t b0 = (a >> bshift) - bbase, b1 = ((lim + ((int64_t)1 << bshift) - 1) >> bshift) - bbase;
    b0 = b0 < 0 ? 0 : (b0 > last ? last : b0);
    b1 = b1 < 0 ? 0 : (b1 > last ? last : b1);
    const uint64_t r0 = a <= 0 ? 0 : (uint64_t)boff[b0], r1 = (uint64_t)boff[b1];
    // (five-row groups: from the 128-byte line that holds the slice's first group -- a wave's 1 KiB load is eight whole lines;
    // six-row groups end at bucket boundaries: the slice is whole groups from its first one)
    const uint64_t g0 = rpg == 6 ? r0 / 6 : (r0 / 5) & ~(uint64_t)7, g1 = (r1 + (uint64_t)rpg - 1) / (uint64_t)rpg;
    TileDesc d;
    d.g0_lo = (uint32_t)g0;
    d.g0_hi = (uint32_t)(g0 >> 32);
    d.ng = r1 - (uint64_t)rpg * g0 >= 0xFFFF0000ull ? 0xFFFFFFFFu : (uint32_t)(g1 - g0);
    d.first = (uint32_t)(r0 - (uint64_t)rpg * g0);
    d.end = (uint32_t)(r1 - (uint64_t)rpg * g0);
    d.g_wrap = 0;
    if (rpg == 6) {  // (bshift 5: buckets of 32 positions)
        const int64_t bw = ((a + 1024) >> bshift) - bbase;
        const uint64_t gw = bw <= 0 ? 0 : (uint64_t)boff[bw > last ? last : bw] / 6;
        d.g_wrap = gw <= g0 ? 0u : (gw - g0 >= 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)(gw - g0));
    }
    d.pad[0] = d.pad[1] = 0;
    out[t] = d;
}

// T = 256: four waves per tile (eight tiles = 32 waves per CU), the only form instantiated (T = 128 lost: see the launcher)
// A9: an index of 256 .. 511 genomes -- the order in the top NINE bits of a level cell (memo_sweep_dense.h: MEMO_ROW9_AT), uint16 results
// AW: the row source is a k-class view whose cap is this k - 1 -- every row of it writes, the row blocks carry no test (memo_sweep_dense.h)
// SIX: the row source is a k-class view in groups of six rows that carry their bucket (memo_view_build.hip: view_build_kernel<6>; the
// library's choice of view where it applies: -2.3 % at k = 31 against five-row views, profiles/r05_view_pass.txt)
// SP: a row source of few rows per tile (under ~3/4 of the 1024 groups a batch of loads covers: the k-class views of config 3, every
// sequence-built index) -- a piece past the tile's slice issues NO load (a wave-uniform branch).  Rounds 3-5 issued all four loads of a
// lane unconditionally, a dead piece fetching one group for its 64 lanes: one request to memory, but a full trip through the
// vector memory pipeline and 1 KiB of registers written, nine to fourteen times per tile at k = 31 ... 9 -- and the sweep is
// sensitive there (four MORE loads per lane, a later tile's rows prefetched into L2, cost it 8-15 %).  Skipping them: k = 31 -3 %,
// k = 21 -3.4 %, k = 17 -4.5 %, k = 9 -6 % on config 3's views.  Not for tiles of several full batches (config 5: +2 ... +6 %:
// behind the branches the compiler waits for ALL of a batch's loads before its first piece), hence a template flag the
// launcher sets from the rows per tile (profiles/r06_headline.txt; masking the dead loads off with EXEC = 0 instead gained nothing).
// LIVE (SIX only): the view's groups say which of them hold no live row (memo_view_build.hip: view_live_kernel) -- a dead group's lane
// sits out its rows' atomics, a piece without a live group is skipped (memo_sweep_dense.h: live_pieces)
// R4 (SIX, not LIVE, k - 1 in [16, 31]): radix-4 level arrays -- blocks of 12, 4 and 1 -- of kLS4 = 1664 cells in place of the five
// doubling arrays of 1024: the same 20 KiB per tile (eight tiles per CU), 1.69x the positions per tile at k = 31 (memo_sweep_dense.h:
// group_rows4; the launcher takes it for six-row views with few rows per tile, launch_halo3t)
template <int NLEV, typename OutT, int T, bool A9 = false, bool AW = false, bool SIX = false, bool SP = false, bool LIVE = false,
          bool R4 = false>
__global__ __launch_bounds__(T) __attribute__((amdgpu_waves_per_eu(T == 256 ? 8 : 4, 8)))
void sweep_conservation_halo3t_kernel(const SweepArgs A) {
    static_assert(!A9 || sizeof(OutT) == 2, "more than 255 genomes: uint16 results");
    static_assert(!(A9 && SIX), "six-row groups hold eight-bit annots");
    static_assert(!LIVE || SIX, "dead-group flags: six-row views");
    static_assert(!R4 || (SIX && !LIVE && NLEV == 5 && T == 256), "radix-4 arrays: six-row views without flags, k - 1 in [16, 31]");
    constexpr int LSZ = R4 ? kLS4 : kLS;  // cells per level array
    constexpr int SH = A9 ? 23 : 24;  // a cell = order << SH | tie-breaking bits
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    constexpr int NL = kStageGroups / T;  // 16-byte groups per lane and batch
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t blk = blockIdx.x;
    const uint32_t tile = (blk & 7u) * (uint32_t)A.tiles_per_xcd + (blk >> 3);  // each XCD group: a contiguous run of tiles
    if (tile >= (uint32_t)A.ntiles) return;
    const uint32_t tabs = (uint32_t)A.tile_abs0 + tile;  // the tile's number in pivot coordinates
    const TileDesc *dp = static_cast<const TileDesc *>(A.ttab) + (tabs < (uint32_t)A.ntab ? tabs : (uint32_t)A.ntab - 1u);
    const uint4 d0 = *reinterpret_cast<const uint4 *>(dp);
    const uint32_t d_end = dp->end, d_wrap = dp->g_wrap;
    Geo g;
    g.g0 = 0;
    g.ng = d0.z;
    g.first = d0.w;
    g.end = d_end;
    if (g.ng == 0xFFFFFFFFu) {
        if (tid == 0) atomicOr(A.status, kStatusHugeSlice);
        return;
    }
    const uint4 *src0 = reinterpret_cast<const uint4 *>(A.p3) + (((uint64_t)d0.y << 32) | d0.x);
    // a lane's four groups of a batch of 1024 (group tid + 256 j): four loads in a row, none under a branch, a piece past the
    // tile's groups loading ONE group for the whole wave (one request) -- or, SP, no load at all for such a piece
    uint4 V[NL];
    auto issue = [&](uint32_t batch) {
#pragma unroll
        for (int j = 0; j < NL; ++j) {
            const uint32_t pg = batch * kStageGroups + (uint32_t)(j * T + wave * 64);
            // (a piece that straddles the slice's end reads up to 63 groups BEHIND the slice -- half a KiB per tile on average: TCP_TCC_READ_REQ
            // is 24 % above a k = 17 view's bytes, profiles/r05_six_rows.txt.  Those are the next tile's first lines, which that tile --
            // same XCD, running beside this one -- fetches anyway: clamping the lanes to the slice's last group measured 0.5-1.5 % SLOWER,
            // same box, alternating builds.)
            uint4 &v = V[j];  // (named before `lane`: the lambda's capture order shapes the compiler's code for the SP kernels)
            const uint32_t at = pg + (uint32_t)lane;
            if constexpr (SP) {
                if (pg < g.ng) v = src0[at];
            } else {
                v = src0[pg < g.ng ? at : 0u];
            }
        }
    };
    issue(0);
    const uint32_t lds_base = (uint32_t)(size_t)(__attribute__((address_space(3))) uint32_t *)lds;
    const int HL = A.hl, W = A.w;
    clear_levels<NLEV, T>(lds_base, cell_sentinel<SH>(A));  // (R4: 3 x 6656 B inside the 20 KiB of five)
    RowConst C;
    C.km1 = A.km1;
    C.status = A.status;
    C.ls4 = 4u * kLS;
    C.bias4 = (uint32_t)pin_vgpr((int)(lds_base + 4u * (uint32_t)HL - (uint32_t)(32 - NLEV) * C.ls4));
    C.top_bit = (uint32_t)pin_vgpr((int)0x80000000u);
    C.a10s = (uint32_t)pin_vgpr((int)(((tabs * (uint32_t)W) & 1023u) << 6));
    SixConst C6;
    C6.km1 = A.km1;
    C6.status = A.status;
    C6.ls4 = R4 ? (uint32_t)(-2 * LSZ) : C.ls4;
    C6.bias4 = R4 ? (uint32_t)pin_vgpr((int)(lds_base + 4u * (uint32_t)HL + 8u * (uint32_t)LSZ)) : C.bias4;
    C6.top_bit = C.top_bit;
    C6.nega = (uint32_t)pin_vgpr((int)((0u - tabs * (uint32_t)W) & 1023u));
    const uint32_t span = g.end - g.first;
    barrier_lds();  // the level arrays are clear

    const uint32_t nbatch = (g.ng + kStageGroups - 1) / kStageGroups;
    for (uint32_t batch = 0; batch == 0 || batch < nbatch; ++batch) {
        if (batch) issue(batch);  // (a tile with more than 5120 rows: the rest)
        const uint32_t gbase = batch * kStageGroups;
        const uint32_t gleft = g.ng > gbase ? g.ng - gbase : 0;
        if constexpr (R4) {
            r4_pieces<T, NL, AW>(V, lane, wave, gleft, d_wrap > gbase ? d_wrap - gbase : 0u, C6);
            continue;
        } else if constexpr (SIX && LIVE) {
            live_pieces<T, NL, AW>(V, lane, wave, gleft, C6);
            continue;
        } else if constexpr (SIX) {
            six_pieces<T, NL, AW>(V, lane, wave, gleft, C6);
            continue;
        }
        // a wave whose four pieces (64 groups each, 256 apart) all lie inside the slice: twenty rows, not one test
        const uint32_t w_row0 = 5u * (gbase + (uint32_t)wave * 64u);
        if (w_row0 >= g.first && w_row0 + 5u * ((uint32_t)(NL - 1) * T + 64u) <= g.end) {
#pragma unroll
            for (int j = 0; j < NL; ++j) group_rows<false, A9, AW>(V[j], C, 0, 0);
            continue;
        }
        reg_pieces<T, NL, 0, A9, AW>(V, tid, wave, gbase, gleft, g, C, span);
    }
    barrier_lds();  // (lgkmcnt(0): the ds_min above are invisible to the compiler)

    // fold in registers + store
    OutT *out = static_cast<OutT *>(A.out);
    const int cells = HL + W;
    // context lanes of a chunk of 64 (R4: the fold of 12s reads two lanes to the left, the fold of 4s one more; 4 * ctx <= hl)
    constexpr int ctx = R4 ? 3 : (NLEV <= 1 ? 0 : (NLEV <= 3 ? 1 : 1 << (NLEV - 3)));
    const int64_t a_rel = (int64_t)tabs * W - A.qs;  // the tile's first position, as an output index
    const int64_t ob = a_rel - HL;
    const int64_t o_lo = a_rel + (tile == 0 ? A.x_lo_first : 0);
    const int64_t o_hi = a_rel + (tile == (uint32_t)A.ntiles - 1u ? A.x_hi_last : W);
    u32x4 L[6];
    auto lv = [&](int i) { return make_uint4(L[i].x, L[i].y, L[i].z, L[i].w); };
    if constexpr (R4) {  // blocks of 12 -> 4 -> positions, in the chunk loop every register fold shares (memo_sweep_fold.h)
        fold_store_chunks<OutT, T, SH>(out, ob, o_lo, o_hi, cells, LSZ, lane, wave, Int<ctx>{}, [&](int xr) {
            read_levels_r4(lds_base + 4u * (uint32_t)xr, L);
            uint4 M = lv(2), M4 = lv(1);
            r4_fold12(M4, lv(0));
            r4_fold4(M, M4);
            return M;
        });
    } else {
        // The doubling arrays: halo_fold_store_dpp of memo_sweep_cons.hip unrolled for NLEV, with the loop and the store of
        // fold_store_chunks / store_cells4 (memo_sweep_fold.h) written out as they were; only the pack is the shared one.  Through
        // the shared loop these kernels came out as the same instructions under another register allocation, and the six-row
        // kernel on config 3's view at k = 31 then took 0.12488 against 0.12255 ms, +1.9 % where the parent's own rounds spread by
        // 1.35 % (k = 9 / 17 / 21: +0.4 / +0.3 / -0.5 %, inside the spread): profiles/fold_tail_refactor.txt, first run.  Written
        // like this every one of them is the parent's code to the instruction (profiles/fold_tail_device_code.txt).
        constexpr int NW = T / 64, valid = 64 - ctx;
        for (int base = wave * 4 * valid; base + 4 * ctx < cells; base += NW * 4 * valid) {
            const int x0 = base + 4 * lane;
            const int xr = x0 < LSZ - 4 ? x0 : LSZ - 4;  // (past the array: lanes whose results are dropped below)
            read_levels<NLEV>(lds_base + 4u * (uint32_t)xr, L);
            uint4 M = lv(0);
            if constexpr (NLEV >= 6) fold_step_dpp<4>(M, lv(NLEV - 5), lane);
            if constexpr (NLEV >= 5) fold_step_dpp<3>(M, lv(NLEV - 4), lane);
            if constexpr (NLEV >= 4) fold_step_dpp<2>(M, lv(NLEV - 3), lane);
            if constexpr (NLEV >= 3) fold_step_dpp<1>(M, lv(NLEV - 2), lane);
            if constexpr (NLEV >= 2) fold_step_dpp<0>(M, lv(NLEV - 1), lane);
            if (lane < ctx || x0 >= cells) continue;
            const int64_t o = ob + x0;
            if (o >= o_lo && o + 4 <= o_hi) {
                store_four(out + o, pack_cells4<OutT, SH>(M));
            } else {
                const uint32_t v[4] = {M.x >> SH, M.y >> SH, M.z >> SH, M.w >> SH};
                for (int i = 0; i < 4; ++i)
                    if (o + i >= o_lo && o + i < o_hi) out[o + i] = (OutT)v[i];
            }
        }
    }
}

// What a wave of a wide tile needs before its row loads and before its barrier, behind one set of names: the leading scalar
// parameters of sweep_conservation_wide_kernel, which gfx950 hands over in SGPRs at wave launch (FlatHead), or the fields of SweepArgs,
// each read where it is used as the kernel above reads them (ArgsHead: sweep_conservation_wide_args_kernel, the A/B of the head).
struct ArgsHead {
    const SweepArgs &A;
    __device__ __forceinline__ const TileDesc *ttab() const { return static_cast<const TileDesc *>(A.ttab); }
    __device__ __forceinline__ const uint4 *rows() const { return reinterpret_cast<const uint4 *>(A.p3); }
    __device__ __forceinline__ uint32_t ntiles() const { return (uint32_t)A.ntiles; }
    __device__ __forceinline__ uint32_t tiles_per_xcd() const { return (uint32_t)A.tiles_per_xcd; }
    __device__ __forceinline__ uint32_t tile_abs0() const { return (uint32_t)A.tile_abs0; }
    __device__ __forceinline__ uint32_t ntab() const { return (uint32_t)A.ntab; }
    __device__ __forceinline__ int hl() const { return A.hl; }
    __device__ __forceinline__ int w() const { return A.w; }
    __device__ __forceinline__ int km1() const { return A.km1; }
    __device__ __forceinline__ int ncols() const { return A.ncols; }
    __device__ __forceinline__ int x_lo_first() const { return A.x_lo_first; }
    __device__ __forceinline__ int x_hi_last() const { return A.x_hi_last; }
};

struct FlatHead {
    const TileDesc *ttab_;
    const uint4 *rows_;
    uint32_t ntiles_, tiles_per_xcd_, tile_abs0_, ntab_;
    int hl_, w_, km1_, ncols_, x_lo_first_, x_hi_last_;
    __device__ __forceinline__ const TileDesc *ttab() const { return ttab_; }
    __device__ __forceinline__ const uint4 *rows() const { return rows_; }
    __device__ __forceinline__ uint32_t ntiles() const { return ntiles_; }
    __device__ __forceinline__ uint32_t tiles_per_xcd() const { return tiles_per_xcd_; }
    __device__ __forceinline__ uint32_t tile_abs0() const { return tile_abs0_; }
    __device__ __forceinline__ uint32_t ntab() const { return ntab_; }
    __device__ __forceinline__ int hl() const { return hl_; }
    __device__ __forceinline__ int w() const { return w_; }
    __device__ __forceinline__ int km1() const { return km1_; }
    __device__ __forceinline__ int ncols() const { return ncols_; }
    __device__ __forceinline__ int x_lo_first() const { return x_lo_first_; }
    __device__ __forceinline__ int x_hi_last() const { return x_hi_last_; }
};

// the parts of the wide-tile kernel's shortened chain (CH; launch_halo3t, memo_tuning.chain_off)
constexpr int kChainFold2 = 1;     // a wave's two fold chunks in flight together
constexpr int kChainInterior = 2;  // tiles off the window's edges store without the window test
// The pair kernel is taken below this many groups per PAIR of wide tiles (launch_halo3t).  Config 3's live copy at k = 31, pairs against
// one tile per workgroup on one index: 179 groups per tile -4.2 %, 239 (10 rows per 100 genome-positions) +0.6 %, 282 (15 per 100)
// +2.1 % -- the threshold stands between the first two (profiles/tile_pairs.txt, section 6).
constexpr double kPairMaxGroups = 418.0;

// The wide tile's body (R4 of the kernel above: radix-4 arrays, six-row views without flags) with the shortened chain, for both of its
// entries.  FLAT: the head came in registers -- the descriptor is then fetched by ONE scalar load of its 32 bytes (written as asm: left
// to itself the compiler splits it, or turns to a vector load and v_readfirstlane).  It is a body of its own: the kernel above, put
// behind a shared __device__ function, came out as other code in every doubling instance (the batch loop counted another way, other
// registers; profiles/tile_chain.txt), and those must stay what they were.
template <typename OutT, bool AW, bool SP, int CH, typename Head>
__device__ __forceinline__ void wide_tile(const SweepArgs &A, const Head &H) {
    constexpr bool FLAT = std::is_same<Head, FlatHead>::value;
    static_assert((FLAT || CH > 0) && CH >= 0 && CH <= (kChainFold2 | kChainInterior), "no part of the chain: the kernel above");
    constexpr int T = 256, LSZ = kLS4, SH = 24;  // (as the kernel above has them for R4)
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    constexpr int NL = kStageGroups / T;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#ifdef MEMO_STAMPS
    unsigned long long stamp_t0 = __builtin_amdgcn_s_memtime();  // entry
#endif
    const uint32_t blk = blockIdx.x;
    const uint32_t tile = (blk & 7u) * H.tiles_per_xcd() + (blk >> 3);
    if (tile >= H.ntiles()) return;
    const uint32_t tabs = H.tile_abs0() + tile;
    const TileDesc *dp = H.ttab() + (tabs < H.ntab() ? tabs : H.ntab() - 1u);
    uint4 d0;
    uint32_t d_wrap;  // (the wide tiles mask by group alone: the slice's rows first .. end come with the same load, unused)
    if constexpr (FLAT) {
        typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
        u32x8 d;
        asm volatile("s_load_dwordx8 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(d) : "s"(dp) : "memory");
        d0 = make_uint4(d[0], d[1], d[2], d[3]);
        d_wrap = d[5];
    } else {
        d0 = *reinterpret_cast<const uint4 *>(dp);
        d_wrap = dp->g_wrap;
    }
    const uint32_t ng = d0.z;
    if (ng == 0xFFFFFFFFu) {
        if (tid == 0) atomicOr(A.status, kStatusHugeSlice);
        return;
    }
    MEMO_STAMP(0);  // the descriptor has arrived
    const uint4 *src0 = H.rows() + (((uint64_t)d0.y << 32) | d0.x);
    uint4 V[NL];
    auto issue = [&](uint32_t batch) {  // (the kernel above says what shaped this)
#pragma unroll
        for (int j = 0; j < NL; ++j) {
            const uint32_t pg = batch * kStageGroups + (uint32_t)(j * T + wave * 64);
            uint4 &v = V[j];
            const uint32_t at = pg + (uint32_t)lane;
            if constexpr (SP) {
                if (pg < ng) v = src0[at];
            } else {
                v = src0[pg < ng ? at : 0u];
            }
        }
    };
    issue(0);
    const uint32_t lds_base = (uint32_t)(size_t)(__attribute__((address_space(3))) uint32_t *)lds;
    const int HL = H.hl(), W = H.w();
    clear_levels<5, T>(lds_base, cell_sentinel<SH>(H.ncols()));  // (3 x 6656 B inside the 20 KiB of five)
    SixConst C6;
    C6.km1 = H.km1();
    C6.status = A.status;
    C6.ls4 = (uint32_t)(-2 * LSZ);
    C6.bias4 = (uint32_t)pin_vgpr((int)(lds_base + 4u * (uint32_t)HL + 8u * (uint32_t)LSZ));
    C6.top_bit = (uint32_t)pin_vgpr((int)0x80000000u);
    C6.nega = (uint32_t)pin_vgpr((int)((0u - tabs * (uint32_t)W) & 1023u));
    barrier_lds();  // the level arrays are clear
    MEMO_STAMP(1);  // first barrier
#ifdef MEMO_STAMPS
    // (wave 0 stamps.  SP: it holds only the loads of its live pieces, one at config 3's ~180 groups per tile, so the wait for all of
    // them is the wait in front of its first group_rows4)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    MEMO_STAMP(2);  // the wave's first row piece is available
#endif

    const uint32_t nbatch = (ng + kStageGroups - 1) / kStageGroups;
    for (uint32_t batch = 0; batch == 0 || batch < nbatch; ++batch) {
        if (batch) issue(batch);
        const uint32_t gbase = batch * kStageGroups;
        const uint32_t gleft = ng > gbase ? ng - gbase : 0;
        r4_pieces<T, NL, AW>(V, lane, wave, gleft, d_wrap > gbase ? d_wrap - gbase : 0u, C6);
    }
    barrier_lds();  // (lgkmcnt(0): the ds_min above are invisible to the compiler)
    MEMO_STAMP(3);  // second barrier

    // fold in registers + store
    OutT *out = static_cast<OutT *>(A.out);
    const int cells = HL + W;
    constexpr int ctx = 3;
    const int64_t a_rel = (int64_t)tabs * W - A.qs;  // the tile's first position, as an output index
    const int64_t ob = a_rel - HL;
    const int64_t o_lo = a_rel + (tile == 0 ? H.x_lo_first() : 0);
    const int64_t o_hi = a_rel + (tile == H.ntiles() - 1u ? H.x_hi_last() : W);
    u32x4 L[6];
    auto lv = [&](int i) { return make_uint4(L[i].x, L[i].y, L[i].z, L[i].w); };
    auto fold1 = [&](int xr) {
        read_levels_r4(lds_base + 4u * (uint32_t)xr, L);
        uint4 M = lv(2), M4 = lv(1);
        r4_fold12(M4, lv(0));
        r4_fold4(M, M4);
        return M;
    };
    if constexpr (CH == 0) {
        fold_store_chunks<OutT, T, SH>(out, ob, o_lo, o_hi, cells, LSZ, lane, wave, Int<ctx>{}, fold1);
    } else {
        // The shortened tail.  A wide tile's cells (at most kLS4) are at most two chunks per wave: a wave that has two reads both
        // chunks' levels before it waits (kChainFold2).  A tile that touches neither edge of the window keeps a lane's quartet iff
        // it lies right of the left halo -- hl, w and a chunk's first cell are multiples of four, no quartet straddles an end --
        // and stores it at a scalar base plus the lane's 32-bit cell number (kChainInterior).
        static_assert(2 * (T / 64) * 4 * (64 - ctx) + 4 * ctx >= kLS4, "a wave of a wide tile: two chunks at the most");
        const bool edge = (tile == 0 && H.x_lo_first() != 0) || (tile == H.ntiles() - 1u && H.x_hi_last() != W);
        OutT *const out_b = out + ob;
        auto fold2 = [&](int xa, int xb, uint4 &Ra, uint4 &Rb) {
            read_levels_r4x2(lds_base + 4u * (uint32_t)xa, lds_base + 4u * (uint32_t)xb, L);
            uint4 M4a = lv(1), M4b = lv(4);
            Ra = lv(2);
            Rb = lv(5);
            r4_fold12(M4a, lv(0));
            r4_fold12(M4b, lv(3));
            r4_fold4(Ra, M4a);
            r4_fold4(Rb, M4b);
        };
        auto tail = [&](auto store) {
            fold_chunks_once_or_twice<T, (CH & kChainFold2) != 0>(cells, LSZ, lane, wave, Int<ctx>{}, fold1, fold2, store);
        };
        auto store_edge = [&](int x0, uint4 R) { store_cells4<OutT, SH>(out, ob + x0, o_lo, o_hi, R); };
        if constexpr ((CH & kChainInterior) != 0) {  // (the wave-uniform choice once, in front of two straight tails)
            if (edge) {
                tail(store_edge);
            } else {
                tail([&](int x0, uint4 R) {
                    if (x0 >= HL) store_four(out_b + (uint32_t)x0, pack_cells4<OutT, SH>(R));
                });
            }
        } else {
            tail(store_edge);
        }
    }
    MEMO_STAMP(4);  // end (the stores issued, not waited for)
#ifdef MEMO_STAMPS
    if (threadIdx.x == 0 && A.stamps) A.stamps[8ull * blockIdx.x + 7] = 1;
#endif
}

// The wide tiles' own entry (R4).  The leading parameters are flat scalars -- a struct by value is not preloaded -- in the order
// of FlatHead: this file is compiled with -amdgpu-kernarg-preload-count=16 (Makefile), and what fits the user SGPRs arrives with
// the wave instead of by a scalar load (a fallback prologue loads it where the firmware does not preload).  FLAT false: the same
// tail parts behind the doubling kernels' signature (A/B: memo_tuning.chain_off).
template <typename OutT, bool AW, bool SP, int CH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8)))
void sweep_conservation_wide_kernel(const TileDesc *ttab, const uint4 *rows, uint32_t ntiles, uint32_t tiles_per_xcd, uint32_t tile_abs0,
                                    uint32_t ntab, int hl, int w, int km1, int ncols, int x_lo_first, int x_hi_last, const SweepArgs A) {
    const FlatHead H = {ttab, rows, ntiles, tiles_per_xcd, tile_abs0, ntab, hl, w, km1, ncols, x_lo_first, x_hi_last};
    wide_tile<OutT, AW, SP, CH>(A, H);
}

template <typename OutT, bool AW, bool SP, int CH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8)))
void sweep_conservation_wide_args_kernel(const SweepArgs A) {
    wide_tile<OutT, AW, SP, CH>(A, ArgsHead{A});
}

// Two wide tiles per workgroup behind one head: the workgroup of pair j sweeps the tiles 2 j and 2 j + 1 of the PIVOT raster (a pair is
// one 64-byte block of the tile table, fetched by one scalar load), one after the other in the same 20 KiB.  Both tiles' rows are
// requested at once, each slice into half of the registers a single tile's batch uses (half a batch, kStageGroups / 2 groups, each;
// every piece begins at its own slice's first group, so the row blocks run as they do in sweep_conservation_wide_kernel, masked in a
// slice's last piece only); then tile A is cleared, scattered, folded and stored, and tile B after it.  One wave launch, one
// descriptor round trip and one round trip of the rows to memory for two tiles; the workgroups stay independent, eight of them
// resident per CU.  A half whose tile lies outside the window (the first pair of a window that starts at an odd tile, the last pair
// of one that ends at an even one) loads, scatters and stores nothing.  A pair with a slice of more than half a batch does its tiles
// as sweep_conservation_wide_kernel does, each with its own loads batch by batch.  The leading parameters are FlatHead's with
// pairs_per_xcd in the place of tiles_per_xcd.  (profiles/tile_pairs.txt: ONE request for the pair's groups, scattered twice under a
// mask, was measured first and is slower than one tile per workgroup -- B's slice begins inside a piece.)
template <typename OutT, bool AW, bool SP, int CH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8)))
void sweep_conservation_wide_pair_kernel(const TileDesc *ttab, const uint4 *rows, uint32_t ntiles, uint32_t pairs_per_xcd, uint32_t tile_abs0,
                                         uint32_t ntab, int hl, int w, int km1, int ncols, int x_lo_first, int x_hi_last, const SweepArgs A) {
    static_assert(SP && CH == (kChainFold2 | kChainInterior), "pairs: few rows per tile, the whole shortened chain");
    constexpr int T = 256, LSZ = kLS4, SH = 24, NL = kStageGroups / T, NH = NL / 2, ctx = 3;
    constexpr uint32_t kHalf = (uint32_t)(NH * T);  // groups of a slice that fit its registers
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t blk = blockIdx.x;
    const uint32_t pair = (blk & 7u) * pairs_per_xcd + (blk >> 3);
    const uint32_t tabs_a = ((tile_abs0 >> 1) + pair) << 1;  // the pair's first tile in pivot coordinates
    const uint32_t rel_a = tabs_a - tile_abs0;               // ... and in the window (2^32 - 1: the tile before its first)
    const bool has_a = rel_a < ntiles, has_b = rel_a + 1u < ntiles;
    if (!has_a && !has_b) return;
    // (ntab is even: tiles past the table's end are its last PAIR, two empty slices)
    const TileDesc *dp = ttab + (tabs_a < ntab - 1u ? tabs_a : ntab - 2u);
    typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
    u32x16 d;
    asm volatile("s_load_dwordx16 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(d) : "s"(dp) : "memory");
    const uint32_t ng_a = d[2], ng_b = d[10], wrap_a = d[5], wrap_b = d[13];
    if ((has_a && ng_a == 0xFFFFFFFFu) || (has_b && ng_b == 0xFFFFFFFFu)) {
        if (tid == 0) atomicOr(A.status, kStatusHugeSlice);
        return;
    }
    const uint4 *src_a = rows + (((uint64_t)d[1] << 32) | d[0]), *src_b = rows + (((uint64_t)d[9] << 32) | d[8]);
    // the window's tiles of this pair, first and (where both halves are present) second: slice, groups, g_wrap
    const uint32_t nh = has_a && has_b ? 2u : 1u;
    const uint4 *src = has_a ? src_a : src_b;
    uint32_t n = has_a ? ng_a : ng_b, wleft = has_a ? wrap_a : wrap_b;
    const bool both = n <= kHalf && (nh == 1u || ng_b <= kHalf);  // the slices fit their registers: requested here, both at once
    uint4 V[NH], VB[NH];  // V: the slice of the tile being swept
    if (both) {
#pragma unroll
        for (int j = 0; j < NH; ++j) {
            const uint32_t pg = (uint32_t)(j * T + wave * 64);
            if (pg < n) V[j] = src[pg + (uint32_t)lane];
        }
#pragma unroll
        for (int j = 0; j < NH; ++j) {
            const uint32_t pg = (uint32_t)(j * T + wave * 64);
            if (nh == 2u && pg < ng_b) VB[j] = src_b[pg + (uint32_t)lane];
        }
    }
    const uint32_t lds_base = (uint32_t)(size_t)(__attribute__((address_space(3))) uint32_t *)lds;
    const int HL = hl, W = w;
    const uint32_t sent = cell_sentinel<SH>(ncols);
    SixConst C6;
    C6.km1 = km1;
    C6.status = A.status;
    C6.ls4 = (uint32_t)(-2 * LSZ);
    C6.bias4 = (uint32_t)pin_vgpr((int)(lds_base + 4u * (uint32_t)HL + 8u * (uint32_t)LSZ));
    C6.top_bit = (uint32_t)pin_vgpr((int)0x80000000u);
    OutT *out = static_cast<OutT *>(A.out);
    const int cells = HL + W;
    u32x4 L[6];
    auto lv = [&](int i) { return make_uint4(L[i].x, L[i].y, L[i].z, L[i].w); };
    auto fold1 = [&](int xr) {
        read_levels_r4(lds_base + 4u * (uint32_t)xr, L);
        uint4 M = lv(2), M4 = lv(1);
        r4_fold12(M4, lv(0));
        r4_fold4(M, M4);
        return M;
    };
    auto fold2 = [&](int xa, int xb, uint4 &Ra, uint4 &Rb) {
        read_levels_r4x2(lds_base + 4u * (uint32_t)xa, lds_base + 4u * (uint32_t)xb, L);
        uint4 M4a = lv(1), M4b = lv(4);
        Ra = lv(2);
        Rb = lv(5);
        r4_fold12(M4a, lv(0));
        r4_fold12(M4b, lv(3));
        r4_fold4(Ra, M4a);
        r4_fold4(Rb, M4b);
    };
    // One tile of the pair per round, from the clear to the store (tabs: its number in pivot coordinates, rel: in the window; V: its
    // slice's groups where they were requested above, else loaded here batch by batch from src).  A loop, not two copies of the body:
    // the row blocks stand once in the code, in front of the fold.
    uint32_t tabs = has_a ? tabs_a : tabs_a + 1u, rel = tabs - tile_abs0;
#pragma unroll 1
    for (uint32_t half = 0; half < nh; ++half) {
        if (half) barrier_lds();  // every wave has read what it folds of the first tile: the arrays may be cleared again
        clear_levels<5, T>(lds_base, sent);
        C6.nega = (uint32_t)pin_vgpr((int)((0u - tabs * (uint32_t)W) & 1023u));
        barrier_lds();  // the level arrays are clear
        if (both) {
            r4_pieces<T, NH, AW>(V, lane, wave, n, wleft, C6);
        } else {
            uint4 VF[NL];
            const uint32_t nbatch = (n + kStageGroups - 1) / kStageGroups;
            for (uint32_t batch = 0; batch < nbatch; ++batch) {
                const uint32_t gbase = batch * kStageGroups, gleft = n - gbase;
#pragma unroll
                for (int j = 0; j < NL; ++j) {
                    const uint32_t pg = (uint32_t)(j * T + wave * 64);
                    VF[j] = src[pg < gleft ? gbase + pg + (uint32_t)lane : 0u];
                }
                r4_pieces<T, NL, AW>(VF, lane, wave, gleft, wleft > gbase ? wleft - gbase : 0u, C6);
            }
        }
        barrier_lds();  // (lgkmcnt(0): the ds_min above are invisible to the compiler)
        const int64_t a_rel = (int64_t)tabs * W - A.qs;  // the tile's first position, as an output index
        const int64_t ob = a_rel - HL;
        const int64_t o_lo = a_rel + (rel == 0 ? x_lo_first : 0);
        const int64_t o_hi = a_rel + (rel == ntiles - 1u ? x_hi_last : W);
        const bool edge = (rel == 0 && x_lo_first != 0) || (rel == ntiles - 1u && x_hi_last != W);
        OutT *const out_b = out + ob;
        auto tail = [&](auto store) { fold_chunks_once_or_twice<T, true>(cells, LSZ, lane, wave, Int<ctx>{}, fold1, fold2, store); };
        if (edge) {
            tail([&](int x0, uint4 R) { store_cells4<OutT, SH>(out, ob + x0, o_lo, o_hi, R); });
        } else {
            tail([&](int x0, uint4 R) {
                if (x0 >= HL) store_four(out_b + (uint32_t)x0, pack_cells4<OutT, SH>(R));
            });
        }
        if (half + 1u < nh) {  // the second tile's
#pragma unroll
            for (int j = 0; j < NH; ++j) V[j] = VB[j];
            src = src_b;
            n = ng_b;
            wleft = wrap_b;
            ++tabs;
            ++rel;
        }
    }
}

}  // namespace

namespace memo {

void drop_tile_tables(memo_index *ix) {  // (callers have the device drained: pack / destroy paths)
    for (memo_index::TileTable &t : ix->ttabs)
        if (t.d) (void)hipFree(t.d);
    ix->ttabs.clear();
}

// the table of (row source, tile width, k): built by the first query that needs it (or by memo_index_prepare), kept with the
// index -- one per combination in use, so that a service that cycles through k classes finds every one of them again
// (round 3 kept four and rebuilt, behind a hipDeviceSynchronize, on the fifth: ADVICE r03); past kMaxTileTables the least
// recently used one is retired (memo_common.h: no wait on the query path)
static int tile_table(memo_index *ix, const void *rows_of, const int64_t *boff, int w, int km1, hipStream_t st, const void **tab,
                      int64_t *ntab, int rpg) {
    memo_index::TileTable *slot = nullptr;
    for (memo_index::TileTable &t : ix->ttabs)
        if (t.d && t.w == w && t.km1 == km1 && t.rows_of == rows_of) slot = &t;
    if (!slot) {
        const int64_t top = ix->max_s < 0 ? 0 : ix->max_s;
        // past the last row: empty slices; an even number of them (the pair kernel fetches the tiles 2 j and 2 j + 1 as one 64-byte block)
        const int64_t n = ((top + km1 + ((int64_t)1 << ix->bshift)) / w + 3 + 1) & ~(int64_t)1;
        if (n >= ((int64_t)1 << 31)) return 1;
        if (ix->ttabs.size() >= kMaxTileTables) {
            size_t lru = 0;
            for (size_t i = 1; i < ix->ttabs.size(); ++i)
                if (ix->ttabs[i].stamp < ix->ttabs[lru].stamp) lru = i;
            retire(ix, ix->ttabs[lru].d, (uint64_t)ix->ttabs[lru].n * sizeof(TileDesc));
            ix->ttabs.erase(ix->ttabs.begin() + (long)lru);
        }
        void *d = nullptr;
        const hipError_t aerr = side_alloc(&d, (size_t)n * sizeof(TileDesc));
        if (aerr == hipErrorOutOfMemory) return kNoRoom;  // (the caller takes the kernel that needs no table)
        HIP_TRY(aerr);
        if ((uintptr_t)d % 64) {  // (device allocations are aligned far beyond this)
            (void)hipFree(d);
            return fail(MEMO_EHIP, "tile table: allocation not aligned to 64 bytes");
        }
        hipLaunchKernelGGL(tile_table_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, boff, (int64_t)ix->nb, ix->bbase,
                           ix->bshift, w, km1, n, static_cast<TileDesc *>(d), rpg);
        hipError_t err = hipGetLastError();
        // complete before this call returns: the next query may come on another stream, and nothing would order its sweep
        // behind this kernel (once per index, tile width and k: some tens of microseconds)
        if (err == hipSuccess) err = hipStreamSynchronize(st);
        if (err != hipSuccess) {
            (void)hipFree(d);
            return fail(MEMO_EHIP, "tile table: %s", hipGetErrorString(err));
        }
        memo_index::TileTable t;
        t.rows_of = rows_of;
        t.w = w;
        t.km1 = km1;
        t.d = d;
        t.n = n;
        ix->ttabs.push_back(t);
        slot = &ix->ttabs.back();
    }
    slot->stamp = ++ix->ttab_clock;
    *tab = slot->d;
    *ntab = slot->n;
    return MEMO_OK;
}

// Launch the table-driven dense-row sweep if this query fits it (else return 1: the caller takes
// sweep_conservation_halo3_kernel).  A: filled for the unclipped sweep (hl, w, ls, nlev, ncols); tw = tile width.
// live: a six-row view whose groups carry the dead-group flag (one built with places)
int launch_halo3t(memo_index *ix, SweepArgs &A, int tw, int elem_bytes, hipStream_t st, bool annot9, bool all_write, bool six, bool live) {
    if (annot9 && elem_bytes != 2) return 1;
    if (six && (annot9 || A.nlev > 5 || ix->bshift != 5)) return 1;
    if (!A.p3 || A.ls > kLS || A.nlev < 1 || A.nlev > 6 || A.km1 > 63 || A.qs < 0) return 1;
    // few rows per tile?  (the rows the sweep reads, spread over the index's span: groups per tile against the 1024 of a batch)
    const double span = (double)(ix->max_s - ix->min_s) + 1.0;
    auto groups_per_tile = [&](int w) { return (double)ix->last_rows_read / (six ? 6.0 : 5.0) * (double)w / (span > 1.0 ? span : 1.0); };
    // R4: the radix-4 arrays in a tile of kLS4 cells (memo_sweep_dense.h), the same halo left and right as the doubling tile's
    const int hl0 = A.hl, w0 = A.w, ls0 = A.ls;
    bool r4 = false;
    if (six && !live && ix->wide_tiles && A.km1 >= 16 && A.km1 <= 31 && A.nlev == 5) {
        const int bw = 1 << ix->bshift, hl = (A.km1 + 3) & ~3, hr = (A.km1 + bw - 1 + 3) & ~3, tw4 = (kLS4 - hl - hr) / bw * bw;
        if (groups_per_tile(tw4) < kR4MaxGroups) {
            r4 = true;
            A.hl = hl;
            A.w = tw = tw4;
            A.ls = hl + tw4 + hr;
        }
    }
    auto no = [&](int rc) {  // (the caller's tile back: it answers with another kernel)
        A.hl = hl0;
        A.w = w0;
        A.ls = ls0;
        return rc;
    };
    const int64_t q = A.qs / tw, tile0 = q * tw;
    const int64_t ntiles = ((A.qe - tile0) + tw - 1) / tw;
    if (ntiles + 8 >= ((int64_t)1 << 31) || q + ntiles >= ((int64_t)1 << 31)) return no(1);
    const void *tab = nullptr;
    int64_t ntab = 0;
    const int rc = tile_table(ix, A.p3, A.boff, tw, A.km1, st, &tab, &ntab, six ? 6 : 5);
    if (rc) return no(rc);
    A.tile0 = tile0;
    A.ntiles = ntiles;
    A.tiles_per_xcd = (ntiles + 7) / 8;
    A.tile_abs0 = q;
    A.ttab = tab;
    A.ntab = ntab;
    A.x_lo_first = (int)(A.qs - tile0);
    A.x_hi_last = (int)(A.qe - (tile0 + (ntiles - 1) * tw));
    // (Two waves per tile, each with twice the rows -- T = 128 -- were tried for row sources with few rows per position, where
    // what a wave does around its rows outweighs the rows: 7-9 % SLOWER on the k-class views of config 3 (0.217 against
    // 0.203 ms at k = 31, 0.168 against 0.154 at k = 17) and 1-4 % slower on all the rows; profiles/r03_views.txt.  Sixteen
    // waves per CU hide the scatter's LDS latency worse than thirty-two, whatever they save in instructions.)
    const bool sp = groups_per_tile(tw) < 768.0;
    // the wide tiles' shortened chain, part by part (memo_tuning.chain_off: all of it in the product)
    const bool flat = r4 && !(ix->tune.chain_off & 1);
    const int chain = r4 ? (~ix->tune.chain_off >> 1) & (kChainFold2 | kChainInterior) : 0;
    // two tiles per workgroup behind one head, where the tiles hold few groups (chain_off & 8: off)
    const bool pairs = flat && chain == (kChainFold2 | kChainInterior) && sp && !(ix->tune.chain_off & 8) && groups_per_tile(2 * tw) < kPairMaxGroups;
    const int64_t npairs = ((q + ntiles + 1) >> 1) - (q >> 1);
    const int64_t per_xcd = pairs ? (npairs + 7) / 8 : A.tiles_per_xcd;  // (workgroups per XCD: of pairs, or of tiles)
    // p: the template arguments as the picker's lambdas are handed them (memo_index::last_pick; kernel: 1 halo3t, 2 wide_args, 3 wide,
    // 4 wide_pair; the caller filled the family, the row format and OutT)
    memo_index::SweepPick p = ix->last_pick;
    p.threads = 256, p.width = tw, p.arrays = A.nlev, p.halo3 = 0;
    SweepKernel kern = pick_int<1, 2, 3, 4, 5, 6>(A.nlev, [&](auto N) {
        return pick_bool(all_write, [&](auto AW) {
            return pick_bool(sp, [&](auto SP) -> SweepKernel {
                p.nlev = N, p.aw = AW, p.sp = SP, p.kernel = 1;
                p.a9 = annot9;
                if (annot9)  // (256 .. 511 genomes: nine-bit orders, uint16 results)
                    return (SweepKernel)sweep_conservation_halo3t_kernel<N, uint16_t, 256, true, AW, false, SP>;
                auto of = [&](auto O) -> SweepKernel {
                    using OutT = typename decltype(O)::type;
                    if constexpr (decltype(N)::value == 5) {
                        if (r4)  // (the flat entry goes through the picker under the doubling kernels' type: cast back at the launch)
                            return pick_int<0, 1, 2, 3>(chain, [&](auto CH) -> SweepKernel {
                                p.six = p.r4 = 1, p.chain = CH;
                                p.kernel = flat ? 3 : decltype(CH)::value == 0 ? 1 : 2;
                                if constexpr (decltype(CH)::value == (kChainFold2 | kChainInterior) && decltype(SP)::value) {
                                    if (pairs) p.pairs = 1, p.kernel = 4;
                                    if (pairs) return reinterpret_cast<SweepKernel>(reinterpret_cast<void (*)()>(sweep_conservation_wide_pair_kernel<OutT, AW, true, CH>));
                                }
                                if (flat) return reinterpret_cast<SweepKernel>(reinterpret_cast<void (*)()>(sweep_conservation_wide_kernel<OutT, AW, SP, CH>));
                                if constexpr (decltype(CH)::value == 0) {
                                    return (SweepKernel)sweep_conservation_halo3t_kernel<5, OutT, 256, false, AW, true, SP, false, true>;
                                } else {
                                    return (SweepKernel)sweep_conservation_wide_args_kernel<OutT, AW, SP, CH>;
                                }
                            });
                    }
                    if constexpr (decltype(N)::value <= 5) {
                        if (six)
                            return pick_bool(live, [&](auto LIVE) {
                                p.six = 1, p.live = LIVE;
                                return (SweepKernel)sweep_conservation_halo3t_kernel<N, OutT, 256, false, AW, true, SP, LIVE>;
                            });
                    }
                    return (SweepKernel)sweep_conservation_halo3t_kernel<N, OutT, 256, false, AW, false, SP>;
                };
                return elem_bytes == 1 ? of(Type<uint8_t>{}) : of(Type<uint16_t>{});
            });
        });
    });
    if (!kern) return no(1);
    ix->last_tile_w = tw;
    ix->last_tiles_per_group = pairs ? 2 : 1;
    ix->last_pick = p;
    if (g_prepare_only) return MEMO_OK;  // memo_index_prepare: the table is built, nothing is launched
    if (int prc = refuse_plan_pointer(A.out)) return prc;
    if (flat) {  // (launch_halo3t's own checks above: the four counts fit 32 bits)
        using WideKernel = void (*)(const TileDesc *, const uint4 *, uint32_t, uint32_t, uint32_t, uint32_t, int, int, int, int, int, int,
                                    const SweepArgs);
        hipLaunchKernelGGL(reinterpret_cast<WideKernel>(reinterpret_cast<void (*)()>(kern)), dim3((unsigned)(per_xcd * 8)), dim3(256), (size_t)A.nlev * 4096, st,
                           static_cast<const TileDesc *>(A.ttab), reinterpret_cast<const uint4 *>(A.p3), (uint32_t)A.ntiles,
                           (uint32_t)per_xcd, (uint32_t)A.tile_abs0, (uint32_t)A.ntab, A.hl, A.w, A.km1, A.ncols, A.x_lo_first,
                           A.x_hi_last, A);
    } else {
        hipLaunchKernelGGL(kern, dim3((unsigned)(A.tiles_per_xcd * 8)), dim3(256), (size_t)A.nlev * 4096, st, A);
    }
    HIP_TRY(hipGetLastError());
    return MEMO_OK;
}

}  // namespace memo
