// memo_ms.hip -- matching statistics of a pivot against genome texts, on the GPU: the stage of `memo index`
// that the reference hands to MONI (src/index.sh:57-80).  One genome at a time:
//
//   suffix array      prefix doubling.  The first sort is on a packed prefix of several characters (the text's
//                     alphabet remapped to the fewest bits); every later round sorts (rank[i], rank[i + h]) as one
//                     64-bit key with rocPRIM's radix sort, and only the suffixes whose group is not yet a singleton
//                     take part.  A head-flag max-scan re-ranks; ranks are "SA position of the group's head + 1", so
//                     finished groups never move.  At most ceil(log2 n) + 2 rounds (host-bounded).
//   ISA, PLCP, LCP    Kärkkäinen-Manzini-Puglisi: PLCP[i] >= PLCP[i-1] - 1, chunk-parallel (every chunk starts its
//                     first position from 0), 8 bytes per compare; LCP[x] = PLCP[SA[x]].
//   min hierarchy     64-ary minima over LCP: "nearest y left / right of x with LCP[y] < t" in a bounded number of
//                     64-entry block scans (2 per level).
//   MS walk           one thread per chunk of pivot positions inside one record, carrying the SA interval of
//                     P[i, i + l): extend by two binary searches on T[SA[y] + l] (direct comparison once the
//                     interval is one suffix), record MS[i] = l, advance through x = ISA[SA[lo] + 1] and the maximal
//                     range around x with LCP >= l - 1.  Exact from any start, so chunks need no fix-up.  An extension
//                     that has taken `budget` steps with more than one suffix left (an N run, a satellite array)
//                     goes on by seed search: a binary search over the SA for the suffix that shares the most with
//                     the rest of the record, 8 bytes per compare, every compare starting at the length the
//                     candidates are known to share (seed_search below).  Same (l, interval), l / 8 reads.
//
//   pieces            a genome given as records (memo_ms_add_records) is uploaded once, back to back, and its text is
//                     assembled on the device piece by piece: each piece a run of whole strings (records, then their
//                     reverse complements), each with its NUL.  No match crosses a NUL, so the MS against the whole
//                     text is the elementwise maximum of the MS against the pieces: the first piece's walk stores,
//                     the later ones store max(M, l).  Every piece stays under the int32 suffix-array limit.
//
// MS columns are written straight into a device DAP matrix int32 [positions][columns] that memo_dap_push_dev
// (memo_dap.hip) consumes in place (the dense layout), or, where that matrix would not fit, into one scratch column
// that is then run-coded (the coded layout, "coded columns" below) and decoded range by range into a staging matrix.
// Bad input sets a device error word that the host turns into an error; nothing traps or spins.  rocPRIM lives in this
// translation unit only (its headers compile slowly).
#include <cstring>  // rocprim's texture iterator calls memset without including it

#include <rocprim/rocprim.hpp>

#include <new>
#include <vector>

#include "memo_common.h"

using namespace memo;

namespace {

constexpr int kPad = 64;          // zero bytes behind the text and the pivot: the 8-byte loads stay inside
constexpr int kFanout = 64;       // min hierarchy: entries per block
constexpr int kMaxLevels = 8;     // 64^6 > 2^31: six levels above LCP at most
constexpr int kLcpChunk = 256;    // text positions per PLCP thread
constexpr int kErrSearch = 1;     // device error bits: a hierarchy search ran off its levels
constexpr int kErrWalk = 2;       //   an MS walk loop hit its bound
constexpr int kErrIsa = 4;        //   an advance step found no successor suffix
constexpr int kBlock = 256;
constexpr int64_t kWalkBudget = 64;              // extension steps before a seed search: the default

unsigned grid_for(int64_t n, int block = kBlock) {  // n < 2^31: at most 2^23 blocks
    const int64_t g = (n + block - 1) / block;
    return (unsigned)(g < 1 ? 1 : g);
}

// 8 bytes starting at byte p (little-endian: byte p is the low byte); two aligned loads and a funnel shift
__device__ __forceinline__ uint64_t load8(const uint8_t *T, int64_t p) {
    const uint64_t *w = reinterpret_cast<const uint64_t *>(T) + (p >> 3);
    const int s = (int)(p & 7) * 8;
    const uint64_t lo = w[0];
    return s ? (lo >> s) | (w[1] << (64 - s)) : lo;
}

// common prefix of A[a, a + lim) and B[b, b + lim), 8 bytes per step; the buffers are padded by kPad.  words: += the 8-byte
// words compared
__device__ __forceinline__ int64_t common_prefix(const uint8_t *A, int64_t a, const uint8_t *B, int64_t b, int64_t lim,
                                                 int64_t &words) {
    int64_t l = 0;
    for (int64_t step = 0; step <= (lim >> 3) && l < lim; ++step) {
        ++words;
        const uint64_t x = load8(A, a + l) ^ load8(B, b + l);
        if (x) {
            l += __builtin_ctzll(x) >> 3;
            break;
        }
        l += 8;
    }
    return l < lim ? l : lim;
}

__device__ __forceinline__ int64_t common_prefix(const uint8_t *A, int64_t a, const uint8_t *B, int64_t b, int64_t lim) {
    int64_t words = 0;
    return common_prefix(A, a, B, b, lim, words);
}

// ---- suffix array ------------------------------------------------------------------------------------

__global__ void histogram_kernel(const uint8_t *T, int64_t n, uint32_t *hist) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        atomicAdd(&h[T[i]], 1u);
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}

struct CharCodes {
    uint16_t code[256];  // 1 .. sigma (sigma <= 256); 0 = past the end of the text
};

// round 0: every suffix, keyed by its first `cpk` characters at `bits` bits each
__global__ void __launch_bounds__(kBlock) prefix_key_kernel(const uint8_t *T, int64_t n, CharCodes cc, int bits, int cpk,
                                                            uint64_t *key, int32_t *suf, int32_t *pos) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t k = 0;
    for (int j = 0; j < cpk; ++j) k = (k << bits) | (i + j < n ? cc.code[T[i + j]] : 0);
    key[i] = k;
    suf[i] = (int32_t)i;
    pos[i] = (int32_t)i;
}

// later rounds: (rank[s], rank[s + h]) of the active suffixes; rank 0 = past the end
__global__ void __launch_bounds__(kBlock) pair_key_kernel(const int32_t *rank, const int32_t *suf, int64_t m, int64_t n, int64_t h,
                                                          int bits, uint64_t *key) {
    const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (j >= m) return;
    const int64_t s = suf[j];
    const uint64_t r2 = s + h < n ? (uint64_t)rank[s + h] : 0;
    key[j] = ((uint64_t)rank[s] << bits) | r2;
}

// after the sort: place the suffixes, flag the group heads (value = SA position + 1 of the head)
__global__ void __launch_bounds__(kBlock) place_kernel(const uint64_t *key, const int32_t *suf, const int32_t *pos, int64_t m,
                                                       int32_t *SA, int32_t *head) {
    const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (j >= m) return;
    SA[pos[j]] = suf[j];
    head[j] = (j == 0 || key[j] != key[j - 1]) ? pos[j] + 1 : 0;
}

// after the max-scan: new ranks; a suffix stays active unless its group is a singleton
__global__ void __launch_bounds__(kBlock) rerank_kernel(const int32_t *head, const int32_t *grp, const int32_t *suf, int64_t m,
                                                        int32_t *rank, int32_t *keep) {
    const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (j >= m) return;
    rank[suf[j]] = grp[j];
    const bool single = head[j] != 0 && (j + 1 == m || head[j + 1] != 0);
    keep[j] = single ? 0 : 1;
}

__global__ void __launch_bounds__(kBlock) compact_kernel(const int32_t *keep, const int32_t *off, const int32_t *suf, const int32_t *pos,
                                                         int64_t m, int32_t *suf_out, int32_t *pos_out) {
    const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (j >= m || !keep[j]) return;
    suf_out[off[j]] = suf[j];
    pos_out[off[j]] = pos[j];
}

// ---- ISA, PLCP, LCP, hierarchy ----------------------------------------------------------------------

__global__ void __launch_bounds__(kBlock) isa_phi_kernel(const int32_t *SA, int64_t n, int32_t *isa, int32_t *phi) {
    const int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (x >= n) return;
    const int32_t s = SA[x];
    isa[s] = (int32_t)x;
    phi[s] = x ? SA[x - 1] : -1;
}

// PLCP over text positions [c * kLcpChunk, (c + 1) * kLcpChunk): the first from 0, the rest from the previous - 1
__global__ void __launch_bounds__(kBlock) plcp_kernel(const uint8_t *T, int64_t n, const int32_t *phi, int32_t *plcp) {
    const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t i0 = c * kLcpChunk;
    if (i0 >= n) return;
    const int64_t i1 = i0 + kLcpChunk < n ? i0 + kLcpChunk : n;
    int64_t l = 0;
    for (int64_t i = i0; i < i1; ++i) {
        const int64_t j = phi[i];
        if (j < 0) {
            l = 0;
        } else {
            const int64_t lim = n - (i > j ? i : j);
            if (l > lim) l = lim;
            l += common_prefix(T, i + l, T, j + l, lim - l);
        }
        plcp[i] = (int32_t)l;
        if (l > 0) --l;
    }
}

__global__ void __launch_bounds__(kBlock) lcp_kernel(const int32_t *SA, const int32_t *plcp, int64_t n, int32_t *lcp) {
    const int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (x >= n) return;
    lcp[x] = x ? plcp[SA[x]] : 0;
}

__global__ void __launch_bounds__(kBlock) block_min_kernel(const int32_t *src, int64_t n_src, int32_t *dst, int64_t n_dst) {
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (e >= n_dst) return;
    const int64_t a = e * kFanout, b = a + kFanout < n_src ? a + kFanout : n_src;
    int32_t m = INT32_MAX;
    for (int64_t y = a; y < b; ++y) m = src[y] < m ? src[y] : m;
    dst[e] = m;
}

struct Hierarchy {
    const int32_t *lv[kMaxLevels];  // lv[0] = LCP
    int64_t size[kMaxLevels];
    int levels;
};

// nearest y <= x with LCP[y] < t, or -1
__device__ int64_t search_left(const Hierarchy &H, int64_t x, int32_t t, int *err) {
    int k = 0;
    int64_t pos = x, found = -1;
    for (; k < H.levels; ++k) {
        const int64_t g0 = pos & ~(int64_t)(kFanout - 1);
        for (int64_t y = pos; y >= g0; --y)
            if (H.lv[k][y] < t) {
                found = y;
                break;
            }
        if (found >= 0 || g0 == 0) break;
        pos = (g0 / kFanout) - 1;
    }
    if (found < 0) {
        if (k >= H.levels) *err |= kErrSearch;
        return -1;
    }
    for (; k > 0; --k) {  // descend: the rightmost child whose minimum is < t
        const int64_t c0 = found * kFanout;
        int64_t c = c0 + kFanout - 1 < H.size[k - 1] ? c0 + kFanout - 1 : H.size[k - 1] - 1;
        for (; c > c0 && H.lv[k - 1][c] >= t; --c) {
        }
        found = c;
    }
    return found;
}

// nearest y >= x with LCP[y] < t, or n
__device__ int64_t search_right(const Hierarchy &H, int64_t x, int32_t t, int *err) {
    if (x >= H.size[0]) return H.size[0];
    int k = 0;
    int64_t pos = x, found = -1;
    for (; k < H.levels; ++k) {
        const int64_t end = (pos | (kFanout - 1)) < H.size[k] - 1 ? (pos | (kFanout - 1)) : H.size[k] - 1;
        for (int64_t y = pos; y <= end; ++y)
            if (H.lv[k][y] < t) {
                found = y;
                break;
            }
        if (found >= 0 || end == H.size[k] - 1) break;
        pos = end / kFanout + 1;
    }
    if (found < 0) {
        if (k >= H.levels) *err |= kErrSearch;
        return H.size[0];
    }
    for (; k > 0; --k) {  // descend: the leftmost child whose minimum is < t
        int64_t c = found * kFanout;
        const int64_t c1 = c + kFanout - 1 < H.size[k - 1] ? c + kFanout - 1 : H.size[k - 1] - 1;
        for (; c < c1 && H.lv[k - 1][c] >= t; ++c) {
        }
        found = c;
    }
    return found;
}

// ---- the walk ------------------------------------------------------------------------------------------

// what the walks of one add call read of the text; a text read is one char_at or one 8-byte word of a common_prefix
struct WalkCounters {
    unsigned long long text_reads, max_chunk_text_reads, seeds, seed_text_reads;
};

struct WalkArgs {
    const uint8_t *T;         // genome text (+ kPad zeros)
    const int32_t *SA, *ISA;
    Hierarchy H;
    int64_t n;
    const uint8_t *P;         // pivot (+ kPad zeros)
    const int64_t *rec_begin; // nrec + 1
    const int64_t *chunk_begin;  // nrec + 1: first walk chunk of each record
    int nrec;
    int64_t chunk;            // positions per walk chunk
    int64_t nchunks;
    int32_t *M;               // DAP [positions][C]
    int C, col;
    int merge;                // 0: store l (the first piece); 1: store max(M, l) (later pieces)
    int64_t budget;           // extension steps at one position before a seed search takes over
    int *err;
    WalkCounters *count;      // summed over the launches of one add call
};

// T[SA[y] + l] as a signed value; -1 past the end of the text (sorts first)
__device__ __forceinline__ int char_at(const WalkArgs &A, int64_t y, int64_t l) {
    const int64_t p = (int64_t)A.SA[y] + l;
    return p < A.n ? (int)A.T[p] : -1;
}

// Seed search.  Every suffix of SA[lo, hi] shares its first l characters with P[i, re).  Returns the one that shares the most
// (x) and sets l to that length: what extending one character at a time arrives at, for the price of l / 8 word compares.
// A binary search over [a, b], which starts as [lo, hi].  `l` is what every suffix of [a, b] is known to share with P[i, re),
// so the compare with the middle suffix m starts there and no character is compared twice.  When m shares k > l, the
// suffixes that share less than k with m (outside the LCP >= k range around m, from the min hierarchy) share less than k
// with the pivot too: [a, b] shrinks to that range and l becomes k.  Then the first characters that differ say on which
// side of m the pivot sorts.  m leaves [a, b] every round and [a, b] at least halves, so 32 rounds do for n < 2^31
// (the bound below allows one more).
__device__ int64_t seed_search(const WalkArgs &A, int64_t i, int64_t re, int64_t lo, int64_t hi, int64_t &l, int64_t &reads,
                               int *err) {
    int64_t a = lo, b = hi, x = lo;
    for (int round = 0; a <= b; ++round) {
        if (round > 32) {
            *err |= kErrWalk;
            break;
        }
        const int64_t m = (a + b) >> 1;
        const int64_t s = A.SA[m];
        const int64_t lim = re - i < A.n - s ? re - i : A.n - s;  // >= l: suffix m shares l characters with P[i, re)
        int64_t k = l;
        if (k < lim) k += common_prefix(A.T, s + k, A.P, i + k, lim - k, reads);
        if (k > l) {
            x = m;
            l = k;
            if (k == re - i) break;  // the rest of the record occurs
            const int64_t y0 = search_left(A.H, m, (int32_t)k, err);
            const int64_t y1 = search_right(A.H, m + 1, (int32_t)k, err);
            a = y0 > a ? y0 : a;
            b = y1 - 1 < b ? y1 - 1 : b;
        }
        ++reads;
        if ((int)A.P[i + k] < char_at(A, m, k)) b = m - 1; else a = m + 1;  // (a suffix that ends here sorts first)
    }
    return x;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o);
        const unsigned long long w = ((unsigned long long)hi << 32) | lo;
        v = w > v ? w : v;
    }
    return v;
}

__global__ void __launch_bounds__(kBlock) ms_walk_kernel(const WalkArgs A) {
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    int err = 0;
    int64_t reads = 0, seeds = 0, seed_reads = 0;  // this chunk's text reads
    if (t < A.nchunks) {
        int lo_r = 0, hi_r = A.nrec;  // record of this chunk: last r with chunk_begin[r] <= t
        while (hi_r - lo_r > 1) {
            const int mid = (lo_r + hi_r) >> 1;
            if (A.chunk_begin[mid] <= t) lo_r = mid; else hi_r = mid;
        }
        const int64_t rb = A.rec_begin[lo_r], re = A.rec_begin[lo_r + 1];
        const int64_t i0 = rb + (t - A.chunk_begin[lo_r]) * A.chunk;
        const int64_t i1 = i0 + A.chunk < re ? i0 + A.chunk : re;
        const int64_t n = A.n;
        int64_t lo = 0, hi = n - 1, l = 0;  // SA interval of P[i, i + l)
        for (int64_t i = i0; i < i1; ++i) {
            // extend
            for (int64_t step = 0; i + l < re; ++step) {
                if (step > re - rb) {
                    err |= kErrWalk;
                    break;
                }
                if (lo == hi) {  // one suffix left: compare directly
                    const int64_t s = A.SA[lo];
                    const int64_t lim = (re - i < n - s ? re - i : n - s);
                    if (l < lim) l += common_prefix(A.T, s + l, A.P, i + l, lim - l, reads);
                    break;
                }
                if (step >= A.budget) {  // still wide after `budget` characters: the rest by seed search
                    const int64_t before = reads;
                    const int64_t x = seed_search(A, i, re, lo, hi, l, reads, &err);
                    ++seeds;
                    seed_reads += reads - before;
                    if (l > 0) {
                        const int64_t y0 = search_left(A.H, x, (int32_t)l, &err);
                        lo = y0 < 0 ? 0 : y0;
                        hi = search_right(A.H, x + 1, (int32_t)l, &err) - 1;
                    } else {
                        lo = 0;
                        hi = n - 1;
                    }
                    break;
                }
                const int c = A.P[i + l];
                int64_t a = lo, b = hi + 1;  // first y in [lo, hi] with char >= c
                for (int k = 0; k < 33 && a < b; ++k) {
                    const int64_t mid = (a + b) >> 1;
                    ++reads;
                    if (char_at(A, mid, l) < c) a = mid + 1; else b = mid;
                }
                if (a > hi) break;  // P[i, i + l] occurs nowhere
                ++reads;
                if (char_at(A, a, l) != c) break;
                int64_t a2 = a, b2 = hi + 1;  // first y in [a, hi] with char > c
                for (int k = 0; k < 33 && a2 < b2; ++k) {
                    const int64_t mid = (a2 + b2) >> 1;
                    ++reads;
                    if (char_at(A, mid, l) <= c) a2 = mid + 1; else b2 = mid;
                }
                lo = a;
                hi = a2 - 1;
                ++l;
            }
            int32_t *m = A.M + i * (int64_t)A.C + A.col;
            *m = A.merge && *m > (int32_t)l ? *m : (int32_t)l;
            // advance: P[i + 1, i + l) is the suffix after SA[lo], less its first character
            if (l > 1) {
                const int64_t s1 = (int64_t)A.SA[lo] + 1;
                if (s1 >= n) {
                    err |= kErrIsa;
                    l = 0;
                    lo = 0;
                    hi = n - 1;
                    continue;
                }
                const int64_t x = A.ISA[s1];
                --l;
                const int64_t y0 = search_left(A.H, x, (int32_t)l, &err);
                const int64_t y1 = search_right(A.H, x + 1, (int32_t)l, &err);
                lo = y0 < 0 ? 0 : y0;
                hi = y1 - 1;
            } else {
                l = 0;
                lo = 0;
                hi = n - 1;
            }
        }
    }
    if (err) atomicOr(A.err, err);
    // the counters: summed (the largest chunk: maximised) over the wave, then one lane adds them
    const unsigned long long r = wave_sum((unsigned long long)reads), rmax = wave_max((unsigned long long)reads);
    const unsigned long long sd = wave_sum((unsigned long long)seeds), sr = wave_sum((unsigned long long)seed_reads);
    if ((threadIdx.x & 63) == 0) {
        WalkCounters *c = A.count;
        if (r) atomicAdd(&c->text_reads, r);
        if (rmax) atomicMax(&c->max_chunk_text_reads, rmax);
        if (sd) atomicAdd(&c->seeds, sd);
        if (sr) atomicAdd(&c->seed_text_reads, sr);
    }
}

// ---- piece texts -----------------------------------------------------------------------------------------

// the complement of `samtools faidx -i` (build_index._COMPLEMENT): A-T, C-G, R-Y, K-M, B-V, D-H; every other byte stays
__device__ __forceinline__ uint8_t complement(uint8_t c) {
    switch (c) {
        case 'A': return 'T';
        case 'T': return 'A';
        case 'C': return 'G';
        case 'G': return 'C';
        case 'R': return 'Y';
        case 'Y': return 'R';
        case 'K': return 'M';
        case 'M': return 'K';
        case 'B': return 'V';
        case 'V': return 'B';
        case 'D': return 'H';
        case 'H': return 'D';
        default: return c;
    }
}

// One piece of S_1 $ ... S_s $ rc(S_1) $ ... rc(S_s) $: strings [s0, s1) into T[0, n), then zeros up to `bytes` (a multiple
// of 8 that covers n + kPad).  R: the records back to back; G[j] (j <= 2 nrec): where string j starts in the whole text, so
// string j is G[j + 1] - G[j] - 1 bytes and record r starts at R[G[r] - r].  Eight output bytes per thread, one 8-byte store.
__global__ void __launch_bounds__(kBlock) piece_text_kernel(const uint8_t *R, const int64_t *G, int nrec, int s0, int s1, int64_t n,
                                                            int64_t bytes, uint8_t *T) {
    const int64_t p0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) * 8;
    if (p0 >= bytes) return;
    uint64_t w = 0;
    if (p0 < n) {
        const int64_t base = G[s0];
        int a = s0, b = s1;  // the last string j with G[j] - base <= p0
        while (b - a > 1) {
            const int mid = (a + b) >> 1;
            if (G[mid] - base <= p0) a = mid; else b = mid;
        }
        int j = a;
        int64_t beg = G[j] - base, end = G[j + 1] - base;  // string j with its NUL: [beg, end)
        for (int k = 0; k < 8 && p0 + k < n; ++k) {
            const int64_t p = p0 + k;
            while (p >= end) {
                ++j;
                beg = end;
                end = G[j + 1] - base;
            }
            const int64_t q = p - beg, len = end - beg - 1;
            uint8_t c = 0;
            if (q < len) {
                const int r = j < nrec ? j : j - nrec;
                const int64_t src = G[r] - r;
                c = j < nrec ? R[src + q] : complement(R[src + len - 1 - q]);
            }
            w |= (uint64_t)c << (8 * k);
        }
    }
    *reinterpret_cast<uint64_t *>(T + p0) = w;
}

template <typename T>
struct DevBuf {  // device buffer that only ever grows
    T *p = nullptr;
    size_t cap = 0;
    int ensure(size_t need) {
        if (need <= cap) return MEMO_OK;
        (void)hipFree(p);
        p = nullptr;
        cap = 0;
        HIP_TRY(hipMalloc(&p, need * sizeof(T)));
        cap = need;
        return MEMO_OK;
    }
    void release() {
        (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// ---- coded columns ---------------------------------------------------------------------------------------
//
// MS[i] >= MS[i - 1] - 1 at every pivot position (inside a record, across record ends, and after the maximum over pieces),
// so a column is known from the positions where it does not simply continue.  The run code of a column:
//   expect[i] = max(MS[i - 1] - 1, 0), MS[-1] = 0;  i is flagged iff MS[i] != expect[i] or i is the first position of a
//   coding block of kCodeBlock positions;  the column is one flag bit per position (64-bit words, bit l of word w = position
//   64 w + l), the int32 MS of every flagged position in position order, and per coding block the rank of its first flag.
//   MS[i] = max(value[j] - (i - j), 0) with j the last flagged position <= i: never further back than the block's start.
// Exact by construction: between two flags every position equals its expect, which is what the decoder replays.

constexpr int kCodeBlock = 2048;                // positions per coding block = per workgroup of the encode kernels
constexpr int kCodeWords = kCodeBlock / 64;     // flag words per coding block
constexpr int kTileCols = 64;                   // decode: columns per workgroup (one 64 x 64 tile through LDS)
constexpr int64_t kLaunchGroups = (int64_t)1 << 22;  // workgroups along x per launch (grid x times block stays below 2^32)
static_assert(kCodeBlock % kBlock == 0 && kBlock == 256 && kCodeWords <= 64, "the encode kernels' shape");

struct CodedRef {  // one column as the decode kernel sees it; flags == nullptr: never added, zeros
    const uint64_t *flags;
    const int64_t *offs;
    const int32_t *vals;
};

// (a) flags and per-block counts.  A workgroup covers one coding block, a wave 64 consecutive positions at a time, so the
// ballot of the flag predicate is the flag word.  Words past the pivot's end are written as 0.
__global__ void __launch_bounds__(kBlock) code_flag_kernel(const int32_t *S, int64_t npos, int64_t blk0, uint64_t *flags,
                                                           int64_t *count) {
    __shared__ int part[kBlock / 64];
    const int64_t blk = blk0 + blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int mine = 0;
    for (int k = 0; k < kCodeBlock / kBlock; ++k) {
        const int64_t i = blk * kCodeBlock + k * kBlock + threadIdx.x;
        bool f = false;
        if (i < npos) {
            const int32_t prev = i > 0 ? S[i - 1] : 0;
            f = S[i] != (prev > 1 ? prev - 1 : 0) || (k == 0 && threadIdx.x == 0);
        }
        const uint64_t w = __ballot(f);
        if (lane == 0) {
            flags[blk * kCodeWords + k * (kBlock / 64) + wave] = w;
            mine += __popcll(w);
        }
    }
    if (lane == 0) part[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
        for (int w = 0; w < kBlock / 64; ++w) c += part[w];
        count[blk] = c;
    }
}

// (d) every flagged value to offs[block] + the flags before it in the block
__global__ void __launch_bounds__(kBlock) code_scatter_kernel(const int32_t *S, int64_t blk0, const uint64_t *flags,
                                                              const int64_t *offs, int32_t *vals) {
    __shared__ int pre[kCodeWords];
    const int64_t blk = blk0 + blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < kCodeWords) pre[threadIdx.x] = __popcll(flags[blk * kCodeWords + threadIdx.x]);
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int k = 0; k < kCodeWords; ++k) {
            const int c = pre[k];
            pre[k] = run;
            run += c;
        }
    }
    __syncthreads();
    const int64_t base = offs[blk];
    for (int k = 0; k < kCodeBlock / kBlock; ++k) {
        const int wi = k * (kBlock / 64) + wave;
        const uint64_t w = flags[blk * kCodeWords + wi];
        if ((w >> lane) & 1)  // a set bit lies inside the pivot (code_flag_kernel)
            vals[base + pre[wi] + __popcll(w & (((uint64_t)1 << lane) - 1))] = S[blk * kCodeBlock + k * kBlock + threadIdx.x];
    }
}

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
    const int lo = __shfl((int)(uint32_t)v, src), hi = __shfl((int)(uint32_t)(v >> 32), src);
    return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}

// Positions [first, first + positions) of all columns into out[positions][C].  A workgroup takes the 64 positions of one flag
// word (absolute, so a range may start and end anywhere) for kTileCols columns: each wave decodes a column at a time, lane =
// position, into an LDS tile, which then goes out row by row -- consecutive threads write consecutive columns of a position.
// The last flag at or before a position: in its own word by count-leading-zeros of the word masked to the lane; else in the
// nearest earlier word of the block that has a bit (lane k holds word k of the block: one ballot finds it).  Its rank: the
// block's offset + the bits of the words before + the bits of the masked word.
__global__ void __launch_bounds__(kBlock) code_decode_kernel(const CodedRef *cols, int C, int64_t first, int64_t positions,
                                                             int64_t tile0, int32_t *out) {
    __shared__ int32_t tile[64 * (kTileCols + 1)];
    const int64_t word = (first >> 6) + tile0 + blockIdx.x;
    const int c0 = blockIdx.y * kTileCols;
    const int nc = C - c0 < kTileCols ? C - c0 : kTileCols;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = word * 64 + lane;
    const bool inside = i >= first && i < first + positions;
    const int64_t blk = word / kCodeWords;
    const int wi = (int)(word % kCodeWords);
    for (int cc = wave; cc < nc; cc += kBlock / 64) {
        const CodedRef col = cols[c0 + cc];
        int32_t v = 0;
        if (col.flags) {  // (the same for the whole wave)
            const uint64_t wk = lane < kCodeWords ? col.flags[blk * kCodeWords + lane] : 0;
            int before = lane < wi ? __popcll(wk) : 0;  // flags of the block ahead of this word
            for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o);
            const uint64_t earlier = __ballot(lane < wi && wk != 0);
            const int kk = earlier ? 63 - __clzll(earlier) : 0;
            const uint64_t wprev = shfl64(wk, kk), w = shfl64(wk, wi);
            const uint64_t m = w & (~(uint64_t)0 >> (63 - lane));
            int64_t j = -1, rank = 0;
            if (m) {
                j = word * 64 + 63 - __clzll(m);
                rank = before + __popcll(m) - 1;
            } else if (earlier) {
                j = (blk * kCodeWords + kk) * 64 + 63 - __clzll(wprev);
                rank = before - 1;
            }
            if (inside && j >= 0) {  // (a block's first position is always flagged: j >= 0 wherever inside)
                const int64_t val = (int64_t)col.vals[col.offs[blk] + rank] - (i - j);
                v = val > 0 ? (int32_t)val : 0;
            }
        }
        tile[lane * (kTileCols + 1) + cc] = v;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < 64 * nc; idx += kBlock) {
        const int p = idx / nc, cc = idx - p * nc;
        const int64_t ii = word * 64 + p;
        if (ii >= first && ii < first + positions) out[(ii - first) * C + c0 + cc] = tile[p * (kTileCols + 1) + cc];
    }
}

// one coded column: the owner of its three allocations (the caller has the handle's device selected)
struct CodedColumn {
    DevPtr<uint64_t> flags;  // kCodeWords words per coding block
    DevPtr<int64_t> offs;    // per coding block: the rank of its first flag
    DevPtr<int32_t> vals;    // `flagged` values
    int64_t flagged = 0;
    int64_t n_flags = 0, n_offs = 0, n_vals = 0;  // elements allocated
    uint64_t bytes() const { return (uint64_t)n_flags * 8 + (uint64_t)n_offs * 8 + (uint64_t)n_vals * 4; }
    void reset() {
        flags.reset(); offs.reset(); vals.reset();
        flagged = n_flags = n_offs = n_vals = 0;
    }
};

int64_t code_blocks(int64_t npos) { return (npos + kCodeBlock - 1) / kCodeBlock; }
// device bytes of one coded column with `flagged` flagged positions: values, flag words, block offsets
int64_t coded_column_bytes(int64_t npos, int64_t flagged) { return 4 * flagged + code_blocks(npos) * (8 * kCodeWords + 8); }

int bits_for(uint64_t v) {  // bits to hold 0 .. v
    int b = 1;
    while (b < 64 && (v >> b)) ++b;
    return b;
}

// the suffix array of T[0, n) (device; T padded by kPad) into SA; the rest is scratch that the caller keeps
struct SaWork {
    DevBuf<uint64_t> key, key2;
    DevBuf<int32_t> suf, suf2, pos, pos2, rank, head, grp;
    DevBuf<uint32_t> hist;
    DevBuf<char> tmp;
    void release() {
        key.release(); key2.release(); suf.release(); suf2.release(); pos.release(); pos2.release();
        rank.release(); head.release(); grp.release(); hist.release(); tmp.release();
    }
};

int build_sa(const uint8_t *dT, int64_t n, int32_t *dSA, SaWork &W, hipStream_t st) {
    int rc;
    const size_t m1 = (size_t)n + 1;
    if ((rc = W.key.ensure(m1)) || (rc = W.key2.ensure(m1)) || (rc = W.suf.ensure(m1)) || (rc = W.suf2.ensure(m1)) ||
        (rc = W.pos.ensure(m1)) || (rc = W.pos2.ensure(m1)) || (rc = W.rank.ensure(m1)) || (rc = W.head.ensure(m1)) ||
        (rc = W.grp.ensure(m1)) || (rc = W.hist.ensure(256)))
        return rc;
    // the text's alphabet, remapped to 1 .. sigma
    HIP_TRY(hipMemsetAsync(W.hist.p, 0, 256 * sizeof(uint32_t), st));
    hipLaunchKernelGGL(histogram_kernel, dim3(grid_for(n) < 1024 ? grid_for(n) : 1024), dim3(256), 0, st, dT, n, W.hist.p);
    HIP_TRY(hipGetLastError());
    uint32_t hist[256];
    HIP_TRY(hipMemcpyAsync(hist, W.hist.p, sizeof(hist), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    CharCodes cc;
    int sigma = 0;
    for (int c = 0; c < 256; ++c) cc.code[c] = hist[c] ? (uint16_t)++sigma : 0;
    const int cbits = bits_for((uint64_t)sigma);
    const int cpk = 64 / cbits;
    // scratch of the radix sort: the largest it will need (the first round sorts all n)
    size_t tmp_bytes = 0;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, tmp_bytes, W.key.p, W.key2.p, W.suf.p, W.suf2.p, (size_t)n, 0, 64, st));
    size_t scan_bytes = 0;
    HIP_TRY(rocprim::inclusive_scan(nullptr, scan_bytes, W.head.p, W.grp.p, (size_t)n, rocprim::maximum<int32_t>(), st));
    tmp_bytes = tmp_bytes > scan_bytes ? tmp_bytes : scan_bytes;
    HIP_TRY(rocprim::exclusive_scan(nullptr, scan_bytes, W.head.p, W.grp.p, (int32_t)0, (size_t)n, rocprim::plus<int32_t>(), st));
    tmp_bytes = tmp_bytes > scan_bytes ? tmp_bytes : scan_bytes;
    if ((rc = W.tmp.ensure(tmp_bytes ? tmp_bytes : 16))) return rc;

    hipLaunchKernelGGL(prefix_key_kernel, dim3(grid_for(n)), dim3(kBlock), 0, st, dT, n, cc, cbits, cpk, W.key.p, W.suf.p, W.pos.p);
    HIP_TRY(hipGetLastError());
    const int rbits = bits_for((uint64_t)n);  // ranks 0 .. n
    int64_t m = n, h = cpk;
    int end_bit = cpk * cbits;
    const int max_rounds = bits_for((uint64_t)n) + 2;  // h grows from >= 1 by doubling: ceil(log2 n) rounds suffice
    for (int round = 0; m > 0; ++round) {
        if (round > max_rounds) return fail(MEMO_EHIP, "suffix array: not done after %d doubling rounds", round);
        if (round > 0) {
            hipLaunchKernelGGL(pair_key_kernel, dim3(grid_for(m)), dim3(kBlock), 0, st, W.rank.p, W.suf.p, m, n, h, rbits, W.key.p);
            HIP_TRY(hipGetLastError());
            h *= 2;
            end_bit = 2 * rbits;
        }
        size_t tb = W.tmp.cap;
        HIP_TRY(rocprim::radix_sort_pairs(W.tmp.p, tb, W.key.p, W.key2.p, W.suf.p, W.suf2.p, (size_t)m, 0, end_bit, st));
        // sorted keys in key2, suffixes in suf2; pos (the ascending SA slots of the active suffixes) stays as it was
        hipLaunchKernelGGL(place_kernel, dim3(grid_for(m)), dim3(kBlock), 0, st, W.key2.p, W.suf2.p, W.pos.p, m, dSA, W.head.p);
        HIP_TRY(hipGetLastError());
        tb = W.tmp.cap;
        HIP_TRY(rocprim::inclusive_scan(W.tmp.p, tb, W.head.p, W.grp.p, (size_t)m, rocprim::maximum<int32_t>(), st));
        int32_t *keep = W.suf.p;  // free since the sort
        hipLaunchKernelGGL(rerank_kernel, dim3(grid_for(m)), dim3(kBlock), 0, st, W.head.p, W.grp.p, W.suf2.p, m, W.rank.p, keep);
        HIP_TRY(hipGetLastError());
        int32_t *off = W.head.p;  // free since the re-rank
        tb = W.tmp.cap;
        HIP_TRY(rocprim::exclusive_scan(W.tmp.p, tb, keep, off, (int32_t)0, (size_t)m, rocprim::plus<int32_t>(), st));
        int32_t last_off = 0, last_keep = 0;
        HIP_TRY(hipMemcpyAsync(&last_off, off + m - 1, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&last_keep, keep + m - 1, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        // the survivors: suffixes into pos2, slots into grp (free since the re-rank); then they become suf / pos
        hipLaunchKernelGGL(compact_kernel, dim3(grid_for(m)), dim3(kBlock), 0, st, keep, off, W.suf2.p, W.pos.p, m, W.pos2.p, W.grp.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
        m = (int64_t)last_off + last_keep;
        std::swap(W.suf, W.pos2);
        std::swap(W.pos, W.grp);
    }
    return MEMO_OK;
}

}  // namespace

struct memo_ms {
    int device = 0, C = 0, nrec = 0;
    int64_t npos = 0;
    int64_t chunk = 0;
    std::vector<int64_t> h_rec_begin, h_G;
    DevBuf<uint8_t> P, T, R;  // R: the records of memo_ms_add_records' genome, back to back
    DevBuf<int64_t> rec_begin, chunk_begin, G;  // G: where each of its strings starts in the whole text
    DevBuf<int32_t> M, SA, ISA, LCP, levels;
    DevBuf<int> err;
    SaWork W;
    float ms_sa = 0.f, ms_lcp = 0.f, ms_walk = 0.f;
    int64_t budget = kWalkBudget;      // of the walks to come (memo_ms_set_walk_budget)
    DevBuf<WalkCounters> walk_count;   // the walks of the add call under way
    memo_ms_walk_info_t walk{};        // of the last add call
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    // the coded layout (M stays empty): the walk's target, the columns, what the encode and decode passes work in
    int layout = MEMO_MS_LAYOUT_DENSE;
    int64_t nblocks = 0;               // coding blocks of the pivot
    DevBuf<int32_t> scratch, stage;    // int32 [positions]: the column being built; [positions asked for][C]: decoded rows
    DevBuf<int64_t> count;             // encode: flags per coding block
    DevBuf<char> scan_tmp;
    DevBuf<CodedRef> refs;             // the columns as the decode kernel reads them (uploaded when refs_stale)
    std::vector<CodedColumn> cols;
    bool refs_stale = true;
    float ms_encode = 0.f, ms_decode = 0.f;
    hipEvent_t cev[2] = {nullptr, nullptr};
};

namespace {

void release(memo_ms *h) {
    h->P.release(); h->T.release(); h->R.release(); h->rec_begin.release(); h->chunk_begin.release(); h->G.release();
    h->M.release(); h->SA.release(); h->ISA.release(); h->LCP.release(); h->levels.release(); h->err.release(); h->walk_count.release();
    h->W.release();
    h->scratch.release(); h->stage.release(); h->count.release(); h->scan_tmp.release(); h->refs.release();
    h->cols.clear();
    for (auto &e : h->ev)
        if (e) (void)hipEventDestroy(e);
    for (auto &e : h->cev)
        if (e) (void)hipEventDestroy(e);
}

int upload_padded(DevBuf<uint8_t> &buf, const uint8_t *src, int64_t n, hipStream_t st) {
    int rc = buf.ensure((size_t)n + kPad);
    if (rc) return rc;
    if (n) HIP_TRY(hipMemcpyAsync(buf.p, src, (size_t)n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(buf.p + n, 0, kPad, st));
    return MEMO_OK;
}

// device bytes a genome text of n characters needs while its suffix array is built (SaWork + SA + text)
uint64_t sa_bytes(int64_t n) { return (uint64_t)n * (8 + 8 + 4 * 9 + 4) + (uint64_t)n / 4 + (64u << 20); }

int fits(int64_t need, const char *what) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if ((uint64_t)need > (uint64_t)free_b)
        return fail(MEMO_EINVAL, "%s needs %.2f GB of device memory, %.2f GB are free (of %.2f GB)", what, need / 1e9,
                    free_b / 1e9, total_b / 1e9);
    return MEMO_OK;
}

// device bytes of one genome text's working set (suffix array, ISA, LCP, hierarchy), and what of it the handle holds already
uint64_t text_bytes(int64_t n) { return sa_bytes(n) + (uint64_t)n * 12 + (uint64_t)n / 8; }
int64_t resident_bytes(const memo_ms *h) {
    return (int64_t)(h->T.cap + (h->SA.cap + h->ISA.cap + h->LCP.cap) * 4 + h->W.key.cap * 16 + h->W.suf.cap * 28);
}

constexpr int64_t kMaxPiece = ((int64_t)1 << 31) - 2;   // int32 suffix array
constexpr int64_t kDefaultPiece = (int64_t)1 << 30;

// strings S_1 .. S_s, rc(S_1) .. rc(S_s) (len + 1 bytes each, the NUL counted) into pieces of at most `cap` bytes, greedily in
// that order; piece_of_string: 2 nrec entries (may be NULL)
int plan_pieces(const int64_t *rec_len, int32_t nrec, int64_t cap, int32_t *piece_of_string, int32_t *pieces) {
    if (nrec < 0 || nrec >= (1 << 30)) return fail(MEMO_EINVAL, "record count %d outside [0, 2^30)", nrec);
    if (cap < 2 || cap > kMaxPiece) return fail(MEMO_EINVAL, "piece cap %lld outside [2, 2^31 - 2]", (long long)cap);
    if (nrec && !rec_len) return fail(MEMO_EINVAL, "rec_len is NULL");
    for (int r = 0; r < nrec; ++r) {
        if (rec_len[r] < 0) return fail(MEMO_EINVAL, "genome record %d has length %lld", r, (long long)rec_len[r]);
        if (rec_len[r] >= cap)  // len + 1 bytes with its NUL
            return fail(MEMO_EINVAL, "genome record %d of %lld bases needs %lld bytes with its separator, more than the piece cap of %lld",
                        r, (long long)rec_len[r], (long long)rec_len[r] + 1, (long long)cap);
    }
    int32_t p = 0;
    int64_t used = 0;
    for (int j = 0; j < 2 * nrec; ++j) {
        const int64_t c = rec_len[j < nrec ? j : j - nrec] + 1;
        if (used + c > cap) {
            ++p;
            used = 0;
        }
        used += c;
        if (piece_of_string) piece_of_string[j] = p;
    }
    if (pieces) *pieces = nrec ? p + 1 : 0;
    return MEMO_OK;
}

// A genome given as records, made ready for its pieces: checked, planned (piece_bytes <= 0: the default cap), its records and
// string offsets G on the device, the buffers of its largest piece allocated.  first[p]: the first string of piece p
// (first[pieces] = 2 nrec).  Nothing of the DAP matrix is touched.
int prepare_records(memo_ms *h, const uint8_t *seq, const int64_t *rec_begin, int32_t nrec, int64_t piece_bytes,
                    std::vector<int32_t> &first, hipStream_t st) {
    if (nrec < 0 || nrec >= (1 << 30)) return fail(MEMO_EINVAL, "record count %d outside [0, 2^30)", nrec);
    if (piece_bytes > kMaxPiece || (piece_bytes > 0 && piece_bytes < 2))
        return fail(MEMO_EINVAL, "piece cap %lld outside [2, 2^31 - 2]", (long long)piece_bytes);
    first.assign(1, 0);
    if (nrec == 0) return MEMO_OK;
    if (!rec_begin) return fail(MEMO_EINVAL, "rec_begin is NULL");
    if (rec_begin[0] != 0) return fail(MEMO_EINVAL, "rec_begin[0] must be 0");
    std::vector<int64_t> len(nrec);
    int64_t longest = 0;
    for (int r = 0; r < nrec; ++r) {
        len[r] = rec_begin[r + 1] - rec_begin[r];
        if (len[r] < 0) return fail(MEMO_EINVAL, "rec_begin is not ascending at record %d", r);
        longest = len[r] > longest ? len[r] : longest;
    }
    const int64_t S = rec_begin[nrec];
    if (S && !seq) return fail(MEMO_EINVAL, "seq is NULL");
    int rc;
    if (piece_bytes > 0 && (rc = plan_pieces(len.data(), nrec, piece_bytes, nullptr, nullptr))) return rc;  // before any upload
    // the records once, back to back; G[j] = where string j starts in the whole text
    std::vector<int64_t> &G = h->h_G;
    G.assign(2 * (size_t)nrec + 1, 0);
    for (int j = 0; j < 2 * nrec; ++j) G[j + 1] = G[j] + len[j < nrec ? j : j - nrec] + 1;
    if ((rc = h->R.ensure((size_t)S + 8)) || (rc = h->G.ensure(G.size()))) return rc;
    if (S) HIP_TRY(hipMemcpyAsync(h->R.p, seq, (size_t)S, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->G.p, G.data(), G.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // the caller's buffer may go once this returns, on any path
    int64_t cap = piece_bytes;
    if (cap <= 0) {  // min(2^30, what the free memory allows), raised to fit the longest string where memory allows
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        uint64_t avail = (uint64_t)free_b + (uint64_t)resident_bytes(h);
        if (h->layout == MEMO_MS_LAYOUT_CODED) {  // the piece's buffers stay while the column is encoded: leave room for the largest
            const uint64_t keep = (uint64_t)coded_column_bytes(h->npos, h->npos) + (uint64_t)code_blocks(h->npos) * 8 + (16u << 20);
            avail = avail > keep ? avail - keep : 0;  // column there can be (every position flagged), the block counts and the scan's scratch
        }
        int64_t n_mem = avail > (64u << 20) ? (int64_t)((avail - (64u << 20)) * 8 / 547) : 0;  // text_bytes(n) ~ 68.375 n + 64 MiB
        while (n_mem > 0 && text_bytes(n_mem) > avail) --n_mem;
        n_mem = n_mem < kMaxPiece ? n_mem : kMaxPiece;
        cap = kDefaultPiece < n_mem ? kDefaultPiece : n_mem;
        if (longest + 1 > cap) cap = longest + 1 < n_mem ? longest + 1 : n_mem;
        cap = cap < 2 ? 2 : cap;
    }
    std::vector<int32_t> piece(2 * (size_t)nrec);
    int32_t pieces = 0;
    if ((rc = plan_pieces(len.data(), nrec, cap, piece.data(), &pieces))) return rc;
    int64_t biggest = 0;
    for (int j = 0; j < 2 * nrec; ++j)
        if (j + 1 == 2 * nrec || piece[j + 1] != piece[j]) {
            first.push_back(j + 1);
            const int64_t n = G[j + 1] - G[first[first.size() - 2]];
            biggest = n > biggest ? n : biggest;
        }
    // the largest piece must fit before the first one writes the column
    const int64_t need = (int64_t)text_bytes(biggest) - resident_bytes(h);
    if (need > 0 && (rc = fits(need, "the largest piece's suffix array and LCP"))) return rc;
    const size_t tbytes = ((size_t)biggest + kPad + 7) & ~(size_t)7;
    if ((rc = h->T.ensure(tbytes)) || (rc = h->SA.ensure(biggest)) || (rc = h->ISA.ensure(biggest)) || (rc = h->LCP.ensure(biggest)))
        return rc;
    return MEMO_OK;
}

// piece [first[p], first[p + 1]) of the prepared genome into h->T (kPad zeros behind it); returns its length
int64_t assemble_piece(memo_ms *h, int32_t nrec, const std::vector<int32_t> &first, int p, hipStream_t st) {
    const int64_t n = h->h_G[first[p + 1]] - h->h_G[first[p]];
    const int64_t bytes = (n + kPad + 7) & ~(int64_t)7;
    hipLaunchKernelGGL(piece_text_kernel, dim3(grid_for(bytes / 8)), dim3(kBlock), 0, st, h->R.p, h->G.p, nrec, first[p],
                       first[p + 1], n, bytes, h->T.p);
    return n;
}

// the suffix array, LCP, hierarchy and walk of the text in h->T[0, n) (padded; SA, ISA, LCP allocated), into `column`:
// stored, or merged by max when `merge`
int ms_of_text(memo_ms *h, int64_t n, int32_t column, int merge, hipStream_t st) {
    int rc;
    HIP_TRY(hipEventRecord(h->ev[0], st));
    if ((rc = build_sa(h->T.p, n, h->SA.p, h->W, st))) return rc;
    HIP_TRY(hipEventRecord(h->ev[1], st));
    // ISA and PHI (PHI in the rank scratch), PLCP (in grp), LCP
    int32_t *phi = h->W.rank.p, *plcp = h->W.grp.p;
    hipLaunchKernelGGL(isa_phi_kernel, dim3(grid_for(n)), dim3(kBlock), 0, st, h->SA.p, n, h->ISA.p, phi);
    hipLaunchKernelGGL(plcp_kernel, dim3(grid_for((n + kLcpChunk - 1) / kLcpChunk)), dim3(kBlock), 0, st, h->T.p, n, phi, plcp);
    hipLaunchKernelGGL(lcp_kernel, dim3(grid_for(n)), dim3(kBlock), 0, st, h->SA.p, plcp, n, h->LCP.p);
    HIP_TRY(hipGetLastError());
    // the min hierarchy over LCP
    Hierarchy H{};
    int64_t sizes[kMaxLevels], offs[kMaxLevels], total = 0;
    int levels = 1;
    sizes[0] = n;
    while (sizes[levels - 1] > 1 && levels < kMaxLevels) {
        sizes[levels] = (sizes[levels - 1] + kFanout - 1) / kFanout;
        offs[levels] = total;
        total += sizes[levels];
        ++levels;
    }
    if ((rc = h->levels.ensure((size_t)(total ? total : 1)))) return rc;
    H.levels = levels;
    H.lv[0] = h->LCP.p;
    H.size[0] = n;
    for (int k = 1; k < levels; ++k) {
        H.lv[k] = h->levels.p + offs[k];
        H.size[k] = sizes[k];
        hipLaunchKernelGGL(block_min_kernel, dim3(grid_for(sizes[k])), dim3(kBlock), 0, st, H.lv[k - 1], sizes[k - 1],
                           h->levels.p + offs[k], sizes[k]);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->ev[2], st));
    // the walk
    WalkArgs A{};
    A.T = h->T.p;
    A.SA = h->SA.p;
    A.ISA = h->ISA.p;
    A.H = H;
    A.n = n;
    A.P = h->P.p;
    A.rec_begin = h->rec_begin.p;
    A.chunk_begin = h->chunk_begin.p;
    A.nrec = h->nrec;
    A.chunk = h->chunk;
    int64_t nchunks = 0;
    for (int r = 0; r < h->nrec; ++r) nchunks += (h->h_rec_begin[r + 1] - h->h_rec_begin[r] + h->chunk - 1) / h->chunk;
    A.nchunks = nchunks;
    const bool coded = h->layout == MEMO_MS_LAYOUT_CODED;  // the walk fills the scratch column; encode_column follows the last piece
    A.M = coded ? h->scratch.p : h->M.p;
    A.C = coded ? 1 : h->C;
    A.col = coded ? 0 : column;
    A.merge = merge;
    A.budget = h->budget;
    A.err = h->err.p;
    A.count = h->walk_count.p;
    HIP_TRY(hipMemsetAsync(h->err.p, 0, sizeof(int), st));
    hipLaunchKernelGGL(ms_walk_kernel, dim3(grid_for(nchunks)), dim3(kBlock), 0, st, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->ev[3], st));
    int errw = 0;
    HIP_TRY(hipMemcpyAsync(&errw, h->err.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    float a = 0, b = 0, c = 0;
    HIP_TRY(hipEventElapsedTime(&a, h->ev[0], h->ev[1]));
    HIP_TRY(hipEventElapsedTime(&b, h->ev[1], h->ev[2]));
    HIP_TRY(hipEventElapsedTime(&c, h->ev[2], h->ev[3]));
    h->ms_sa += a;
    h->ms_lcp += b;
    h->ms_walk += c;
    if (errw) return fail(MEMO_EHIP, "matching statistics of column %d: the walk kernel reported error bits 0x%x", column, errw);
    return MEMO_OK;
}

// an add call's counters: cleared before its first piece, read after its last
int begin_add(memo_ms *h, hipStream_t st) {
    h->walk = memo_ms_walk_info_t{};
    h->walk.budget = h->budget;
    HIP_TRY(hipMemsetAsync(h->walk_count.p, 0, sizeof(WalkCounters), st));
    return MEMO_OK;
}

int end_add(memo_ms *h, hipStream_t st) {
    WalkCounters c{};
    HIP_TRY(hipMemcpyAsync(&c, h->walk_count.p, sizeof c, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    h->walk.text_reads = c.text_reads;
    h->walk.max_chunk_text_reads = c.max_chunk_text_reads;
    h->walk.seeds = c.seeds;
    h->walk.seed_text_reads = c.seed_text_reads;
    return MEMO_OK;
}

// ---- layouts ---------------------------------------------------------------------------------------------

// what memo_ms_create asks of the free memory: the matrix, the pivot, the working set of a 1 MiB text
int64_t dense_need(int64_t npos, int64_t columns) { return npos * columns * 4 + npos + (int64_t)sa_bytes(1 << 20); }
// the least a coded handle can hold: the scratch column, the pivot, every column's flag words and block offsets (no values
// yet), the same working set
int64_t coded_floor(int64_t npos, int64_t columns) {
    return npos * 4 + npos + kPad + columns * coded_column_bytes(npos, 0) + (int64_t)sa_bytes(1 << 20);
}

// The layout decision (memo_ms_plan_layout; memo_ms_create_layout with the device's figures).  total_bytes 0: not known.
int plan_layout(int64_t npos, int32_t columns, uint64_t free_b, uint64_t total_b, int32_t layout, int32_t *chosen, int64_t *floor_bytes) {
    if (layout != MEMO_MS_LAYOUT_AUTO && layout != MEMO_MS_LAYOUT_DENSE && layout != MEMO_MS_LAYOUT_CODED)
        return fail(MEMO_EINVAL, "layout %d: 0 = auto, 1 = dense, 2 = coded", layout);
    if (columns < 1 || columns > 4096) return fail(MEMO_EINVAL, "columns must be in [1, 4096], got %d", columns);
    if (npos < 1 || npos >= ((int64_t)1 << 40)) return fail(MEMO_EINVAL, "pivot of %lld positions: need 1 .. 2^40 - 1", (long long)npos);
    const int64_t dense = dense_need(npos, columns), floor = coded_floor(npos, columns);
    const bool dense_fits = (uint64_t)dense <= free_b, coded_fits = (uint64_t)floor <= free_b;
    int pick = layout;
    if (layout == MEMO_MS_LAYOUT_AUTO) pick = dense_fits || !coded_fits ? MEMO_MS_LAYOUT_DENSE : MEMO_MS_LAYOUT_CODED;
    const int64_t need = pick == MEMO_MS_LAYOUT_DENSE ? dense : floor;
    if (chosen) *chosen = pick;
    if (floor_bytes) *floor_bytes = need;
    if (pick == MEMO_MS_LAYOUT_DENSE ? dense_fits : coded_fits) return MEMO_OK;
    char of[48] = "";
    if (total_b) snprintf(of, sizeof of, " (of %.2f GB)", total_b / 1e9);
    if (layout == MEMO_MS_LAYOUT_AUTO)
        return fail(MEMO_EINVAL, "the DAP needs %.2f GB of device memory even as coded columns (%.2f GB as a matrix), %.2f GB are free%s",
                    floor / 1e9, dense / 1e9, free_b / 1e9, of);
    return fail(MEMO_EINVAL, "%s needs %.2f GB of device memory, %.2f GB are free%s",
                pick == MEMO_MS_LAYOUT_DENSE ? "the DAP matrix" : "the coded DAP (scratch column, flag words, block offsets)", need / 1e9,
                free_b / 1e9, of);
}

// one allocation of coded column `column`: refused with the column, the bytes asked for and the bytes free when it does not fit
template <typename T>
int column_alloc(DevPtr<T> &buf, int64_t &held, int64_t n, int32_t column, const char *what) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (memo::g_ms_free_bytes >= 0) free_b = (size_t)memo::g_ms_free_bytes;  // (AB library: memo_debug_ms_free_bytes)
    const uint64_t bytes = (uint64_t)(n > 0 ? n : 1) * sizeof(T);
    if (bytes > free_b || buf.alloc((size_t)(n > 0 ? n : 1)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(MEMO_EHIP, "coded column %d: its %s need %llu bytes of device memory, %llu bytes are free", column, what,
                    (unsigned long long)bytes, (unsigned long long)free_b);
    }
    held = n > 0 ? n : 1;
    return MEMO_OK;
}

int encode_passes(memo_ms *h, CodedColumn &col, int32_t column, hipStream_t st) {
    const int64_t nb = h->nblocks;
    int rc;
    if ((rc = h->count.ensure((size_t)nb))) return rc;
    if ((rc = column_alloc(col.flags, col.n_flags, nb * kCodeWords, column, "flag words")) ||
        (rc = column_alloc(col.offs, col.n_offs, nb, column, "block offsets")))
        return rc;
    HIP_TRY(hipEventRecord(h->cev[0], st));
    for (int64_t b0 = 0; b0 < nb; b0 += kLaunchGroups)
        hipLaunchKernelGGL(code_flag_kernel, dim3((unsigned)(nb - b0 < kLaunchGroups ? nb - b0 : kLaunchGroups)), dim3(kBlock), 0, st,
                           h->scratch.p, h->npos, b0, col.flags.p, h->count.p);
    HIP_TRY(hipGetLastError());
    size_t tmp = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, tmp, h->count.p, col.offs.p, (int64_t)0, (size_t)nb, rocprim::plus<int64_t>(), st));
    if ((rc = h->scan_tmp.ensure(tmp ? tmp : 16))) return rc;
    HIP_TRY(rocprim::exclusive_scan(h->scan_tmp.p, tmp, h->count.p, col.offs.p, (int64_t)0, (size_t)nb, rocprim::plus<int64_t>(), st));
    int64_t last_off = 0, last_count = 0;
    HIP_TRY(hipMemcpyAsync(&last_off, col.offs.p + nb - 1, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&last_count, h->count.p + nb - 1, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t total = last_off + last_count;
    if (total < nb || total > h->npos) return fail(MEMO_EHIP, "coded column %d: %lld flags counted over %lld positions", column, (long long)total, (long long)h->npos);
    if ((rc = column_alloc(col.vals, col.n_vals, total, column, "flagged values"))) return rc;
    for (int64_t b0 = 0; b0 < nb; b0 += kLaunchGroups)
        hipLaunchKernelGGL(code_scatter_kernel, dim3((unsigned)(nb - b0 < kLaunchGroups ? nb - b0 : kLaunchGroups)), dim3(kBlock), 0, st,
                           h->scratch.p, b0, col.flags.p, col.offs.p, col.vals.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->cev[1], st));
    HIP_TRY(hipStreamSynchronize(st));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, h->cev[0], h->cev[1]));
    h->ms_encode += ms;
    col.flagged = total;
    return MEMO_OK;
}

// the scratch column into coded column `column`, whose earlier content goes first; on failure the column is left as one never
// added (zeros, no storage) and the handle stays good
int encode_column(memo_ms *h, int32_t column, hipStream_t st) {
    CodedColumn &col = h->cols[column];
    col.reset();
    h->refs_stale = true;
    const int rc = encode_passes(h, col, column, st);
    if (rc) col.reset();
    return rc;
}

// a genome that matches nothing: a column of zeros
int zero_column(memo_ms *h, int32_t column, hipStream_t st) {
    if (h->layout == MEMO_MS_LAYOUT_CODED) {
        HIP_TRY(hipMemsetAsync(h->scratch.p, 0, (size_t)h->npos * sizeof(int32_t), st));
        return encode_column(h, column, st);
    }
    HIP_TRY(hipMemset2D(h->M.p + column, (size_t)h->C * 4, 0, 4, (size_t)h->npos));
    return MEMO_OK;
}

// DAP rows [first, first + positions) of a coded handle into h->stage, done on return
int decode_rows(memo_ms *h, int64_t first, int64_t positions, hipStream_t st) {
    int rc;
    if ((rc = h->stage.ensure((size_t)(positions * h->C > 0 ? positions * h->C : 1)))) return rc;
    if (!positions) return MEMO_OK;
    if (h->refs_stale) {
        std::vector<CodedRef> refs(h->C);
        for (int c = 0; c < h->C; ++c) refs[c] = CodedRef{h->cols[c].flags.p, h->cols[c].offs.p, h->cols[c].vals.p};
        if ((rc = h->refs.ensure((size_t)h->C))) return rc;
        HIP_TRY(hipMemcpy(h->refs.p, refs.data(), refs.size() * sizeof(CodedRef), hipMemcpyHostToDevice));
        h->refs_stale = false;
    }
    const int64_t tiles = ((first + positions - 1) >> 6) - (first >> 6) + 1;
    const unsigned groups = (unsigned)((h->C + kTileCols - 1) / kTileCols);
    HIP_TRY(hipEventRecord(h->cev[0], st));
    for (int64_t t0 = 0; t0 < tiles; t0 += kLaunchGroups)
        hipLaunchKernelGGL(code_decode_kernel, dim3((unsigned)(tiles - t0 < kLaunchGroups ? tiles - t0 : kLaunchGroups), groups), dim3(kBlock),
                           0, st, h->refs.p, h->C, first, positions, t0, h->stage.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->cev[1], st));
    HIP_TRY(hipStreamSynchronize(st));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, h->cev[0], h->cev[1]));
    h->ms_decode += ms;
    return MEMO_OK;
}

}  // namespace

thread_local int64_t memo::g_ms_free_bytes = -1;

int memo::ms_piece_text(memo_ms_t *h, const uint8_t *seq, const int64_t *rec_begin, int32_t nrec, int64_t piece_bytes, int32_t piece,
                        uint8_t *out, int64_t out_cap, int64_t *out_n) {
    if (!h || !out_n) return fail(MEMO_EINVAL, "NULL argument");
    OnDevice on(h->device, OnDevice::kSelectOnly);
    if (on.rc) return on.rc;
    hipStream_t st = nullptr;
    std::vector<int32_t> first;
    int rc = prepare_records(h, seq, rec_begin, nrec, piece_bytes, first, st);
    if (rc) return rc;
    const int np = (int)first.size() - 1;
    if (piece < 0 || piece >= np) return fail(MEMO_EINVAL, "piece %d outside [0, %d)", piece, np);
    const int64_t n = assemble_piece(h, nrec, first, piece, st);
    HIP_TRY(hipGetLastError());
    *out_n = n;
    if (out && n + kPad <= out_cap) HIP_TRY(hipMemcpyAsync(out, h->T.p, (size_t)(n + kPad), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return np;
}

extern "C" {

int memo_suffix_array(const uint8_t *text, int64_t n, int32_t *sa_out, int32_t device) {
    if (n < 0 || n >= ((int64_t)1 << 31) - 1) return fail(MEMO_EINVAL, "text length %lld outside [0, 2^31 - 1)", (long long)n);
    if (n == 0) return MEMO_OK;
    if (!text || !sa_out) return fail(MEMO_EINVAL, "NULL argument");
    OnDevice on(device, OnDevice::kSelectOnly);
    if (on.rc) return on.rc;
    int rc = fits((int64_t)sa_bytes(n), "the suffix array");
    if (rc) return rc;
    DevBuf<uint8_t> T;
    DevBuf<int32_t> SA;
    SaWork W;
    hipStream_t st = nullptr;
    rc = upload_padded(T, text, n, st);
    if (!rc) rc = SA.ensure((size_t)n);
    if (!rc) rc = build_sa(T.p, n, SA.p, W, st);
    if (!rc && hipMemcpy(sa_out, SA.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
        rc = fail(MEMO_EHIP, "memo_suffix_array: copy back failed");
    T.release();
    SA.release();
    W.release();
    return rc;
}

void memo_ms_destroy(memo_ms_t *h) {
    if (!h) return;
    DeviceGuard guard(h->device);
    release(h);
    delete h;
}

int memo_ms_create(const uint8_t *pivot, const int64_t *rec_begin, int32_t nrec, int32_t columns, int64_t chunk,
                   int32_t device, memo_ms_t **out) {
    return memo_ms_create_layout(pivot, rec_begin, nrec, columns, chunk, device, MEMO_MS_LAYOUT_DENSE, out);
}

int memo_ms_plan_layout(int64_t positions, int32_t columns, uint64_t free_bytes, int32_t layout, int32_t *chosen, int64_t *floor_bytes) {
    return plan_layout(positions, columns, free_bytes, 0, layout, chosen, floor_bytes);
}

int memo_ms_create_layout(const uint8_t *pivot, const int64_t *rec_begin, int32_t nrec, int32_t columns, int64_t chunk,
                          int32_t device, int32_t layout, memo_ms_t **out) {
    if (!out) return fail(MEMO_EINVAL, "out is NULL");
    *out = nullptr;
    if (columns < 1 || columns > 4096) return fail(MEMO_EINVAL, "columns must be in [1, 4096], got %d", columns);
    if (nrec < 1 || !rec_begin) return fail(MEMO_EINVAL, "need at least one pivot record");
    if (rec_begin[0] != 0) return fail(MEMO_EINVAL, "rec_begin[0] must be 0");
    for (int r = 0; r < nrec; ++r) {
        const int64_t L = rec_begin[r + 1] - rec_begin[r];
        if (L < 1 || L >= ((int64_t)1 << 30))
            return fail(MEMO_EINVAL, "pivot record %d has length %lld (need 1 .. 2^30-1)", r, (long long)L);
    }
    const int64_t npos = rec_begin[nrec];
    if (npos >= ((int64_t)1 << 40)) return fail(MEMO_EINVAL, "pivot of %lld positions is too long", (long long)npos);
    if (chunk <= 0) chunk = 128;
    if (chunk > ((int64_t)1 << 30)) return fail(MEMO_EINVAL, "walk chunk %lld too long", (long long)chunk);
    OnDevice on(device, OnDevice::kSelectOnly);
    if (on.rc) return on.rc;
    // the DAP (dense: the matrix; coded: the scratch column and every column's flags) stays resident; every genome's working set
    // comes on top of it
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    int32_t chosen = 0;
    int rc = plan_layout(npos, columns, free_b, total_b, layout, &chosen, nullptr);
    if (rc) return rc;
    if (!pivot) return fail(MEMO_EINVAL, "pivot is NULL");
    if (memchr(pivot, 0, (size_t)npos)) return fail(MEMO_EINVAL, "the pivot holds a NUL byte");
    memo_ms *h = new (std::nothrow) memo_ms();
    if (!h) return fail(MEMO_EHIP, "out of host memory");
    h->device = device;
    h->C = columns;
    h->nrec = nrec;
    h->npos = npos;
    h->chunk = chunk;
    h->h_rec_begin.assign(rec_begin, rec_begin + nrec + 1);
    std::vector<int64_t> cb(nrec + 1, 0);
    for (int r = 0; r < nrec; ++r) cb[r + 1] = cb[r] + (rec_begin[r + 1] - rec_begin[r] + chunk - 1) / chunk;
    hipStream_t st = nullptr;
    rc = upload_padded(h->P, pivot, npos, st);
    if (!rc) rc = h->rec_begin.ensure((size_t)nrec + 1);
    if (!rc) rc = h->chunk_begin.ensure((size_t)nrec + 1);
    const bool coded = chosen == MEMO_MS_LAYOUT_CODED;
    h->layout = chosen;
    h->nblocks = code_blocks(npos);
    if (coded) h->cols.resize((size_t)columns);  // (no device storage until a column is added)
    if (!rc) rc = coded ? h->scratch.ensure((size_t)npos) : h->M.ensure((size_t)(npos * columns));
    if (!rc) rc = h->err.ensure(1);
    if (!rc) rc = h->walk_count.ensure(1);
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemcpy(h->rec_begin.p, rec_begin, (nrec + 1) * sizeof(int64_t), hipMemcpyHostToDevice);
    if (!rc && e == hipSuccess) e = hipMemcpy(h->chunk_begin.p, cb.data(), (nrec + 1) * sizeof(int64_t), hipMemcpyHostToDevice);
    if (!rc && e == hipSuccess)
        e = coded ? hipMemset(h->scratch.p, 0, (size_t)npos * sizeof(int32_t)) : hipMemset(h->M.p, 0, (size_t)(npos * columns) * sizeof(int32_t));
    for (auto &ev : h->ev)
        if (!rc && e == hipSuccess) e = hipEventCreate(&ev);
    for (auto &ev : h->cev)
        if (!rc && e == hipSuccess && coded) e = hipEventCreate(&ev);
    if (!rc && e == hipSuccess) e = hipDeviceSynchronize();
    if (rc || e != hipSuccess) {
        memo_ms_destroy(h);
        return rc ? rc : fail(MEMO_EHIP, "memo_ms_create: %s", hipGetErrorString(e));
    }
    *out = h;
    return MEMO_OK;
}

int memo_ms_add_genome(memo_ms_t *h, const uint8_t *text, int64_t n, int32_t column) {
    if (!h) return fail(MEMO_EINVAL, "handle is NULL");
    if (column < 0 || column >= h->C) return fail(MEMO_EINVAL, "column %d outside [0, %d)", column, h->C);
    if (n < 0 || n >= ((int64_t)1 << 31) - 1)
        return fail(MEMO_EINVAL, "genome text of %lld characters: the limit is 2^31 - 2 (int32 suffix array)", (long long)n);
    OnDevice on(h->device, OnDevice::kSelectOnly);
    if (on.rc) return on.rc;
    hipStream_t st = nullptr;
    int rc = begin_add(h, st);
    if (rc) return rc;
    if (n == 0) return zero_column(h, column, st);  // an empty genome matches nothing: its column is zero
    if (!text) return fail(MEMO_EINVAL, "text is NULL");
    // what is not allocated yet must fit (the buffers grow only)
    const int64_t need = (int64_t)text_bytes(n) - resident_bytes(h);
    if (need > 0 && (rc = fits(need, "this genome's suffix array and LCP"))) return rc;
    if ((rc = upload_padded(h->T, text, n, st)) || (rc = h->SA.ensure(n)) || (rc = h->ISA.ensure(n)) ||
        (rc = h->LCP.ensure(n)))
        return rc;
    if ((rc = ms_of_text(h, n, column, 0, st)) || (rc = end_add(h, st))) return rc;
    return h->layout == MEMO_MS_LAYOUT_CODED ? encode_column(h, column, st) : MEMO_OK;
}

int memo_ms_plan_pieces(const int64_t *rec_len, int32_t nrec, int64_t cap, int32_t *piece_of_string, int32_t *pieces) {
    return plan_pieces(rec_len, nrec, cap, piece_of_string, pieces);
}

int memo_ms_add_records(memo_ms_t *h, const uint8_t *seq, const int64_t *rec_begin, int32_t nrec, int32_t column,
                        int64_t piece_bytes, int32_t *pieces) {
    if (!h) return fail(MEMO_EINVAL, "handle is NULL");
    if (column < 0 || column >= h->C) return fail(MEMO_EINVAL, "column %d outside [0, %d)", column, h->C);
    OnDevice on(h->device, OnDevice::kSelectOnly);
    if (on.rc) return on.rc;
    hipStream_t st = nullptr;
    std::vector<int32_t> first;
    int rc = prepare_records(h, seq, rec_begin, nrec, piece_bytes, first, st);
    if (rc || (rc = begin_add(h, st))) return rc;
    const int np = (int)first.size() - 1;
    if (np == 0 && (rc = zero_column(h, column, st))) return rc;  // no records: the text is empty and matches nothing
    for (int p = 0; p < np; ++p) {
        const int64_t n = assemble_piece(h, nrec, first, p, st);
        HIP_TRY(hipGetLastError());
        if ((rc = ms_of_text(h, n, column, p > 0, st))) return rc;
    }
    if ((rc = end_add(h, st))) return rc;
    if (np && h->layout == MEMO_MS_LAYOUT_CODED && (rc = encode_column(h, column, st))) return rc;
    if (pieces) *pieces = np;
    return MEMO_OK;
}

int memo_ms_fetch(memo_ms_t *h, int64_t first, int64_t positions, int32_t *out) {
    if (!h) return fail(MEMO_EINVAL, "handle is NULL");
    if (first < 0 || positions < 0 || first + positions > h->npos)
        return fail(MEMO_EINVAL, "positions [%lld, %lld) outside the pivot's %lld", (long long)first,
                    (long long)(first + positions), (long long)h->npos);
    if (!positions) return MEMO_OK;
    if (!out) return fail(MEMO_EINVAL, "out is NULL");
    DeviceGuard guard(h->device);
    if (h->layout == MEMO_MS_LAYOUT_CODED) {  // through the staging buffer, 256 MiB of rows at a time
        const int64_t step = ((int64_t)64 << 20) / h->C;
        for (int64_t done = 0; done < positions; done += step) {
            const int64_t n = positions - done < step ? positions - done : step;
            if (int rc = decode_rows(h, first + done, n, nullptr)) return rc;
            HIP_TRY(hipMemcpy(out + done * h->C, h->stage.p, (size_t)(n * h->C) * sizeof(int32_t), hipMemcpyDeviceToHost));
        }
        return MEMO_OK;
    }
    HIP_TRY(hipMemcpy(out, h->M.p + first * h->C, (size_t)(positions * h->C) * sizeof(int32_t), hipMemcpyDeviceToHost));
    return MEMO_OK;
}

int memo_ms_push_dap(memo_ms_t *h, memo_dap_t *dap, int64_t first, int64_t positions, uint64_t *out_rows) {
    if (!h || !dap || !out_rows) return fail(MEMO_EINVAL, "NULL argument");
    if (first < 0 || positions < 0 || first + positions > h->npos)
        return fail(MEMO_EINVAL, "positions [%lld, %lld) outside the pivot's %lld", (long long)first,
                    (long long)(first + positions), (long long)h->npos);
    int dev = -1, cols = 0;
    dap_shape(dap, &dev, &cols);
    if (dev != h->device || cols != h->C)
        return fail(MEMO_EINVAL, "the DAP handle has %d columns on device %d, the matching statistics %d on device %d", cols, dev,
                    h->C, h->device);
    if (h->layout == MEMO_MS_LAYOUT_CODED) {  // decoded and waited for before the push reads it
        DeviceGuard guard(h->device);
        if (int rc = decode_rows(h, first, positions, nullptr)) return rc;
        return memo_dap_push_dev(dap, h->stage.p, positions, out_rows);
    }
    return memo_dap_push_dev(dap, h->M.p + first * h->C, positions, out_rows);
}

int memo_ms_rows_dev(memo_ms_t *h, int64_t first, int64_t positions, const int32_t **d_rows) {
    if (!h || !d_rows) return fail(MEMO_EINVAL, "NULL argument");
    if (first < 0 || positions < 0 || first + positions > h->npos)
        return fail(MEMO_EINVAL, "positions [%lld, %lld) outside the pivot's %lld", (long long)first,
                    (long long)(first + positions), (long long)h->npos);
    *d_rows = nullptr;
    if (!positions) return MEMO_OK;
    if (h->layout == MEMO_MS_LAYOUT_CODED) {  // decoded and waited for before the caller reads it
        DeviceGuard guard(h->device);
        if (int rc = decode_rows(h, first, positions, nullptr)) return rc;
        *d_rows = h->stage.p;
        return MEMO_OK;
    }
    *d_rows = h->M.p + first * h->C;
    return MEMO_OK;
}

int memo_ms_layout_info(memo_ms_t *h, memo_ms_layout_info_t *info) {
    if (!h || !info) return fail(MEMO_EINVAL, "NULL argument");
    memset(info, 0, sizeof *info);
    info->layout = h->layout;
    info->block = kCodeBlock;
    info->dense_bytes = (uint64_t)h->npos * (uint64_t)h->C * 4;
    if (h->layout == MEMO_MS_LAYOUT_CODED) {
        info->device_bytes = (uint64_t)(h->scratch.cap + h->stage.cap) * 4;
        for (const CodedColumn &col : h->cols)
            if (col.flags.p) {  // what the column's three allocations hold, not the formula
                info->device_bytes += col.bytes();
                info->flagged += (uint64_t)col.flagged;
            }
    } else {
        info->device_bytes = (uint64_t)h->M.cap * 4;
    }
    info->encode_ms = h->ms_encode;
    info->decode_ms = h->ms_decode;
    return MEMO_OK;
}

int memo_ms_column_info(memo_ms_t *h, int32_t column, uint64_t *flagged, uint64_t *bytes) {
    if (!h) return fail(MEMO_EINVAL, "handle is NULL");
    if (column < 0 || column >= h->C) return fail(MEMO_EINVAL, "column %d outside [0, %d)", column, h->C);
    const bool coded = h->layout == MEMO_MS_LAYOUT_CODED;
    const bool held = coded && h->cols[column].flags.p;
    if (flagged) *flagged = held ? (uint64_t)h->cols[column].flagged : 0;
    if (bytes) *bytes = coded ? (held ? h->cols[column].bytes() : 0) : (uint64_t)h->npos * 4;
    return MEMO_OK;
}

int memo_ms_set_walk_budget(memo_ms_t *h, int64_t steps) {
    if (!h) return fail(MEMO_EINVAL, "handle is NULL");
    h->budget = steps < 0 ? kWalkBudget : steps;  // (2^30 or more: no extension takes that many steps)
    return MEMO_OK;
}

int memo_ms_walk_info(memo_ms_t *h, memo_ms_walk_info_t *info) {
    if (!h || !info) return fail(MEMO_EINVAL, "NULL argument");
    *info = h->walk;
    return MEMO_OK;
}

int memo_ms_timings(memo_ms_t *h, float *out3) {
    if (!h || !out3) return fail(MEMO_EINVAL, "NULL argument");
    out3[0] = h->ms_sa;
    out3[1] = h->ms_lcp;
    out3[2] = h->ms_walk;
    return MEMO_OK;
}

}  // extern "C"
