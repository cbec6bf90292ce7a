// memo_index.hip -- the resident index and its life: error plumbing; birth (new_index), the row-change rule (rows_changed) and the
// rows with end < start; create / upload / truncate / columns / finalize / pack / pack_dense and the overlap census; info and
// options; prepare; synthetic rows.  Two small index-free jobs live here too: `memo view` binning and the four memo_dev_* helpers.
// (The one-shot host forms are memo_oneshot.hip, the builder and export / import memo_hostpack.hip, the views memo_view.hip.)
//
// Counterpart of the arrays /root/reference/src/memo_query.py hands from filter_pq to memo_init
// (:28-36, :45): three int64 columns, kept in HBM so that many windows reuse one upload.
#include <cstdarg>
#include <exception>
#include <cstddef>
#include <new>

#include "memo_view.h"

using namespace memo;

extern "C" __attribute__((visibility("hidden"))) int memo_sort_rows_by_start(int64_t *s, int64_t *e, int64_t *o, uint64_t rows,
                                       uint64_t padded_rows, hipStream_t stream, char *err,
                                       size_t errcap);

namespace {

// ------------------------------------------------------------------------------------------
// kernels: validation, padding and the bucket table (finalize); the 4-byte words and the dense rows (pack, pack_dense); the
// overlap census; `memo view` binning; synthetic rows
// ------------------------------------------------------------------------------------------
__global__ void check_rows_kernel(const int64_t *s, const int64_t *e, uint64_t rows,
                                  uint64_t *scratch) {
    uint64_t unsorted = 0, longrow = 0, wild = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < rows;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const int64_t si = s[i], ei = e[i];
        if (i > 0 && s[i - 1] > si) ++unsorted;
        if (ei < si) ++longrow;
        if (si <= -kCoordLimit || si >= kCoordLimit || ei <= -kCoordLimit || ei >= kCoordLimit) ++wild;
    }
    if (unsorted) atomicAdd((unsigned long long *)&scratch[0], (unsigned long long)unsorted);
    if (longrow) atomicAdd((unsigned long long *)&scratch[1], (unsigned long long)longrow);
    if (wild) atomicAdd((unsigned long long *)&scratch[2], (unsigned long long)wild);
}

__global__ void pad_rows_kernel(int64_t *s, int64_t *e, int64_t *o, uint64_t rows, uint64_t padded) {
    const uint64_t i = rows + blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i < padded) {
        s[i] = kSentinel;
        e[i] = kSentinel;
        o[i] = 0;
    }
}

// finalize: copy the rows with end < start aside (order is irrelevant: min / and commute)
__global__ void collect_long_rows_kernel(const int64_t *s, const int64_t *e, const int64_t *o, uint64_t rows,
                                         int64_t *ls, int64_t *le, int64_t *lo, unsigned long long *count) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < rows;
         i += (uint64_t)gridDim.x * blockDim.x)
        if (e[i] < s[i]) {
            const unsigned long long k = atomicAdd(count, 1ull);
            ls[k] = s[i];
            le[k] = e[i];
            lo[k] = o[i];
        }
}

// memo_index_pack: annot range census, then one word (+ optional 16-bit annot) per row
// (step > 1: a SAMPLE, every step-th row -- memo_index_pack guesses the word layout from it and packs at once; the packing kernel
// takes the exact census on the way: reading the annot column twice was 0.85 ms of config 3's packing pass)
__global__ void annot_census_kernel(const int64_t *o, uint64_t rows, uint64_t *scratch, uint64_t step) {
    uint64_t outside = 0, over8 = 0, top = 0;
    for (uint64_t i = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) * step; i < rows;
         i += (uint64_t)gridDim.x * blockDim.x * step) {
        const int64_t v = o[i];
        if (v < 0 || v > 65535) ++outside;
        else if ((uint64_t)v > top) top = (uint64_t)v;
        if (v > 255) ++over8;
    }
    if (outside) atomicAdd((unsigned long long *)&scratch[3], (unsigned long long)outside);
    if (over8) atomicAdd((unsigned long long *)&scratch[4], (unsigned long long)over8);
    if (top) atomicMax((unsigned long long *)&scratch[5], (unsigned long long)top);
}

// fmt: 4 = start16 | len8 << 16 | annot8 << 24;  12 = len8 | start12 << 8 | annot12 << 20;  6 = the first word with
// annot 0 + a 16-bit annot column  (PackedRows, memo_sweep.h)
// ... and, with `census`, what annot_census_kernel counts, of every row: scratch[3] annots outside [0, 65535], [5] the largest
__global__ void pack_rows_kernel(const int64_t *s, const int64_t *e, const int64_t *o, uint64_t rows,
                                 uint64_t padded, uint32_t *pk, uint16_t *pa, int fmt, uint64_t *census) {
    uint64_t outside = 0, top = 0;
    auto word = [&](uint64_t i, int64_t si, int64_t ei, int64_t v, uint32_t &a) -> uint32_t {
        uint32_t w = 0;
        a = 0;
        if (i < rows) {
            const int64_t len = ei - si;
            // end < start (handled by long_rows_kernel) packs as "never writes", like len >= 255
            const uint32_t l8 = (uint32_t)(len > 255 || len < 0 ? 255 : len);
            if (v < 0 || v > 65535) ++outside;
            else if ((uint64_t)v > top) top = (uint64_t)v;
            a = (uint32_t)v;
            w = fmt == 12 ? l8 | (((uint32_t)si & 0xFFFu) << 8) | (a << 20) : ((uint32_t)si & 0xFFFFu) | (l8 << 16);
        }
        if (fmt == 4) w |= a << 24;
        return w;
    };
    // two rows per lane and load (16 bytes of each column; `padded` is a multiple of 16 rows and the columns are that long), two
    // such pairs in flight: 24 B in, 4 B out per row at 5.1 TB/s with one row per lane and load (2.75 ms per 5 * 10^8 rows)
    const uint64_t stride = 2 * (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = 2 * (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x); i < padded; i += 2 * stride) {
        const uint64_t j = i + stride;
        const bool two = j < padded;
        longlong2 S0 = make_longlong2(0, 0), E0 = S0, O0 = S0, S1 = S0, E1 = S0, O1 = S0;
        // (read once, never again: non-temporal, so that 12 GB of columns do not sweep the L2 and the Infinity Cache)
        auto load2 = [](const int64_t *p) {
            longlong2 v;
            v.x = __builtin_nontemporal_load(p);
            v.y = __builtin_nontemporal_load(p + 1);
            return v;
        };
        if (i < rows) {  // (behind the last row only the words' zeros are written: an empty index has no columns at all)
            S0 = load2(s + i);
            E0 = load2(e + i);
            O0 = load2(o + i);
        }
        if (j < rows) {
            S1 = load2(s + j);
            E1 = load2(e + j);
            O1 = load2(o + j);
        }
        uint32_t a0, a1;
        const uint32_t w0 = word(i, S0.x, E0.x, O0.x, a0), w1 = word(i + 1, S0.y, E0.y, O0.y, a1);
        *reinterpret_cast<uint2 *>(pk + i) = make_uint2(w0, w1);
        if (fmt == 6) *reinterpret_cast<uint32_t *>(pa + i) = a0 | (a1 << 16);
        if (two) {
            const uint32_t w2 = word(j, S1.x, E1.x, O1.x, a0), w3 = word(j + 1, S1.y, E1.y, O1.y, a1);
            *reinterpret_cast<uint2 *>(pk + j) = make_uint2(w2, w3);
            if (fmt == 6) *reinterpret_cast<uint32_t *>(pa + j) = a0 | (a1 << 16);
        }
    }
    if (census) {  // one pair of atomics per wave
        for (int off = 32; off; off >>= 1) {
            const uint64_t t = (uint64_t)__shfl_xor((long long)top, off, 64);
            top = t > top ? t : top;
            outside += (uint64_t)__shfl_xor((long long)outside, off, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            if (outside) atomicAdd((unsigned long long *)&census[3], (unsigned long long)outside);
            if (top) atomicMax((unsigned long long *)&census[5], (unsigned long long)top);
        }
    }
}

// memo_index_pack_dense: 4-byte words -> dense rows, five per 16-byte group (layout: PackedRows3, memo_sweep.h).
// f12: the words are format 12 (overlap | start << 8 | annot << 20) with annots of up to NINE bits: the ninth bit of row i's
// annot goes to bit 16 + i of the group's last dword (the byte no row used while annots had eight)
__global__ void pack3_rows_kernel(const uint32_t *pk, uint64_t padded, uint64_t groups, uint4 *p3, int f12) {
    for (uint64_t g = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; g < groups;
         g += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t B[5], A[5], hi = 0;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const uint32_t x = 5 * g + i < padded ? pk[5 * g + i] : 0u;
            const uint32_t len = f12 ? x & 0xFFu : (x >> 16) & 0xFFu, start = f12 ? x >> 8 : x, annot = f12 ? (x >> 20) & 0x1FFu : x >> 24;
            B[i] = ((start & 1023u) << 6) | (len > 63u ? 63u : len);  // (start & 1023) << 6 | min(length, 63)
            A[i] = annot & 0xFFu;
            hi |= (annot >> 8) << i;
        }
        p3[g] = make_uint4(B[0] | ((B[4] & 0xFFu) << 16) | (A[0] << 24), B[1] | ((B[4] >> 8) << 16) | (A[1] << 24),
                           B[2] | (A[4] << 16) | (A[2] << 24), B[3] | (hi << 16) | (A[3] << 24));
    }
}

// boff[b] = lower_bound(start, b << shift); the last bucket is pinned to `rows`
__global__ void bucket_table_kernel(const int64_t *s, uint64_t rows, int64_t *boff, uint64_t nb,
                                    int shift) {
    const uint64_t b = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (b >= nb) return;
    if (b == nb - 1) {
        boff[b] = (int64_t)rows;
        return;
    }
    const int64_t key = (int64_t)(b << shift);
    uint64_t lo = 0, hi = rows;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (s[mid] < key) lo = mid + 1; else hi = mid;
    }
    boff[b] = (int64_t)lo;
}

// one workgroup per sampled block of 1024 rows: LDS histogram of the overlap byte, then its non-empty bins to HBM
__global__ __launch_bounds__(256) void len_census_kernel(const uint32_t *__restrict__ pk, uint64_t rows, int shift,
                                                         uint64_t step, unsigned int *__restrict__ hist) {
    __shared__ unsigned int h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t r = ((uint64_t)blockIdx.x * step * 256 + threadIdx.x) * 4;
    if (r < rows) {  // (pk is padded: the 16 bytes are there)
        const uint4 v = *reinterpret_cast<const uint4 *>(pk + r);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        for (int i = 0; i < 4; ++i)
            if (r + i < rows) atomicAdd(&h[(w[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}

// the same for dense rows: one workgroup per sampled block of 256 groups (1280 rows)
__global__ __launch_bounds__(256) void dense_census_kernel(const uint4 *__restrict__ p3, uint64_t rows, uint64_t step,
                                                           unsigned int *__restrict__ hist) {
    __shared__ unsigned int h[64];
    if (threadIdx.x < 64) h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t g = (uint64_t)blockIdx.x * step * 256 + threadIdx.x;
    if (5 * g < rows) {
        const uint4 v = p3[g];
        const uint32_t len[5] = {v.x & 63u, v.y & 63u, v.z & 63u, v.w & 63u, (v.x >> 16) & 63u};
        for (int i = 0; i < 5; ++i)
            if (5 * g + i < rows) atomicAdd(&h[len[i]], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 64 && h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}

// which overlap values (min(end - start, 255)) occur among ALL the rows: one pass, a flag per value in LDS (plain stores: lanes
// that hit the same flag merge), the workgroup's flags or-ed into eight words in HBM
__global__ __launch_bounds__(256) void len_seen_kernel(const uint32_t *__restrict__ pk, uint64_t rows, int shift,
                                                       unsigned int *__restrict__ seen) {
    __shared__ uint32_t flag[256];
    flag[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t r = 4 * (blockIdx.x * (uint64_t)256 + threadIdx.x); r < rows; r += 4 * (uint64_t)gridDim.x * 256) {
        const uint4 v = *reinterpret_cast<const uint4 *>(pk + r);  // (pk is padded: the 16 bytes are there)
        flag[(v.x >> shift) & 255u] = 1u;
        if (r + 1 < rows) flag[(v.y >> shift) & 255u] = 1u;
        if (r + 2 < rows) flag[(v.z >> shift) & 255u] = 1u;
        if (r + 3 < rows) flag[(v.w >> shift) & 255u] = 1u;
    }
    __syncthreads();
    // one atomic per word and workgroup (a flag per thread was 60 atomics per workgroup on the same two words of HBM: 5 * 10^5 of
    // them, one after the other in the L2 -- 5.0 of this pass's 5.0 ms on 5 * 10^8 rows)
    const unsigned long long b = __ballot(flag[threadIdx.x] != 0);
    if ((threadIdx.x & 63) == 0) {
        const unsigned int lo = (unsigned int)b, hi = (unsigned int)(b >> 32), w = threadIdx.x >> 5;
        if (lo) atomicOr(&seen[w], lo);
        if (hi) atomicOr(&seen[w + 1], hi);
    }
}

// `memo view` binning (plot_conservation.py:52-56): counts[b][v] = #{p in [edge[b], edge[b+1]) : vec[p] == v}
// for v in 0..num_docs.  One workgroup per (bin, slice of the bin); LDS histogram when it fits.
template <bool LDS_HIST>
__global__ __launch_bounds__(256) void bin_conservation_kernel(const uint16_t *vec, const int64_t *edges,
                                                               int ncols, int slices,
                                                               unsigned long long *counts) {
    extern __shared__ uint32_t hist[];
    const int b = blockIdx.x / slices, sl = blockIdx.x % slices;
    const int64_t lo = edges[b], hi = edges[b + 1];
    const int64_t per = (hi - lo + slices - 1) / slices;
    const int64_t p0 = lo + sl * per, p1 = p0 + per < hi ? p0 + per : hi;
    if (LDS_HIST) {
        for (int i = threadIdx.x; i < ncols; i += 256) hist[i] = 0;
        __syncthreads();
    }
    for (int64_t p = p0 + threadIdx.x; p < p1; p += 256) {
        const int v = vec[p];
        if (v < ncols) {
            if (LDS_HIST) atomicAdd(&hist[v], 1u);
            else atomicAdd(&counts[(int64_t)b * ncols + v], 1ull);
        }
    }
    if (LDS_HIST) {
        __syncthreads();
        for (int i = threadIdx.x; i < ncols; i += 256)
            if (hist[i]) atomicAdd(&counts[(int64_t)b * ncols + i], (unsigned long long)hist[i]);
    }
}

__device__ __forceinline__ uint64_t mix64(uint64_t seed, uint64_t x) {
    uint64_t z = seed + (x + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ void synth_rows_kernel(int64_t *s, int64_t *e, int64_t *o, uint64_t rows,
                                  uint64_t row_begin, uint64_t num, uint64_t den, uint64_t nm1,
                                  uint64_t seed) {
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < rows;
         j += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = row_begin + j;
        const int64_t st = 1 + (int64_t)((i * den) / num);
        s[j] = st;
        e[j] = st + (int64_t)(mix64(seed, 2 * i) % 60);
        o[j] = 1 + (int64_t)(mix64(seed, 2 * i + 1) % nm1);
    }
}

}  // namespace

namespace memo {

// ------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------
thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

int device_ok(int device) {
    const int ndev = memo_device_count();
    return device >= 0 && device < ndev ? MEMO_OK : fail(MEMO_EHIP, "HIP device %d not available (%d visible)", device, ndev);
}

int need_wide(const memo_index *ix) {
    return ix->has_wide ? MEMO_OK : fail(MEMO_EINVAL, "the int64 columns of this index were dropped by memo_index_pack");
}

// ------------------------------------------------------------------------------------------
// the life of an index: its one birth, and what a change of its rows makes stale
// ------------------------------------------------------------------------------------------
int new_index(uint64_t rows, int device, hipStream_t st, memo_index **out) {
    OnDevice on(device);
    if (on.rc) return on.rc;
    memo_index *ix = new (std::nothrow) memo_index();
    if (!ix) return fail(MEMO_EHIP, "out of host memory");
    ix->device = device;
    ix->rows = rows;
    ix->padded = padded_for(rows);
    hipError_t err = ix->d_status.alloc(16);
    if (err == hipSuccess) err = ix->d_scratch.alloc(8);
    if (err == hipSuccess) err = st ? hipMemsetAsync(ix->d_status, 0, 64, st) : hipMemset(ix->d_status, 0, 64);
    if (err != hipSuccess) {
        memo_index_destroy(ix);
        return fail(MEMO_EHIP, "the status words of a new index: %s", hipGetErrorString(err));
    }
    *out = ix;
    return MEMO_OK;
}

void rows_changed(memo_index *ix, Level at, bool keep_word_buffers) {
    if (at <= kLevelDense) {
        drop_tile_tables(ix);  // (all of them, before the views: drop_dense_views then finds none to retire)
        ix->p3.reset();
        ix->boff3.reset();
        ix->rows3 = ix->padded3 = 0;
    }
    drop_dense_views(ix);
    if (at != kLevelDense) drop_packed_views(ix);  // (new dense rows are made of the same words)
    if (at <= kLevelWords) {
        ix->packed_fmt = 0;
        if (!keep_word_buffers) {
            ix->pk.reset();
            ix->pa.reset();
            ix->packed_rows = 0;
        }
    }
    if (at == kLevelColumns) ix->finalized = 0;
}

}  // namespace memo

// ------------------------------------------------------------------------------------------
// the rows with end < start
// ------------------------------------------------------------------------------------------
hipError_t memo_index::LongRows::set(const int64_t *host, uint64_t rows, hipStream_t st) {
    n = 0;
    cols.reset();
    if (!rows) return hipSuccess;
    hipError_t err = cols.alloc(3 * rows);
    if (err == hipSuccess) err = hipMemcpyAsync(cols.p, host, 3 * rows * sizeof(int64_t), hipMemcpyHostToDevice, st);
    if (err == hipSuccess) n = rows;
    return err;
}

int memo_index::LongRows::collect(const memo_index *ix, uint64_t found, hipStream_t st) {
    n = 0;
    cols.reset();
    if (!found) return MEMO_OK;
    if (found > ((uint64_t)1 << 22))
        return fail(MEMO_ELONGROW, "%llu rows have end < start: not a MEMO overlap index", (unsigned long long)found);
    HIP_TRY(cols.alloc(3 * found));
    HIP_TRY(hipMemsetAsync(ix->d_scratch + 6, 0, 8, st));
    const unsigned grid = (unsigned)(ix->rows / 256 + 1 < 4096 ? ix->rows / 256 + 1 : 4096);
    hipLaunchKernelGGL(collect_long_rows_kernel, dim3(grid), dim3(256), 0, st, ix->s, ix->e, ix->o, ix->rows, cols.p, cols.p + found,
                       cols.p + 2 * found, (unsigned long long *)(ix->d_scratch + 6));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    n = found;
    return MEMO_OK;
}

int memo_index::LongRows::download(int device, int64_t *host) const {
    if (!n) return MEMO_OK;
    DeviceGuard guard(device);
    HIP_TRY(hipMemcpy(host, cols, 3 * n * sizeof(int64_t), hipMemcpyDeviceToHost));
    return MEMO_OK;
}

// ------------------------------------------------------------------------------------------
// the overlap census
// ------------------------------------------------------------------------------------------
int memo_len_census(memo_index *ix) {
    ix->len_hist_rows = 0;
    ix->len_seen_exact = 0;
    for (unsigned int &c : ix->len_seen) c = 0;
    for (unsigned int &c : ix->len_hist) c = 0;
    if (!ix->rows) return MEMO_OK;
    // an index that holds the dense rows only (the builder's dense way in, memo_index_import_dense): the same sampled
    // histogram from their 6-bit overlap fields (63 = "63 or more") -- what the rule that decides when a k-class view is
    // worth its pass (memo_view.hip: view_due) estimates the view's size from
    const bool dense_only = !ix->pk && ix->p3;
    const uint64_t drows = ix->boff3 ? ix->rows3 : ix->rows, groups = (drows + 4) / 5;
    if (dense_only ? !groups : (!ix->pk || (ix->packed_fmt != 4 && ix->packed_fmt != 6 && ix->packed_fmt != 12))) return MEMO_OK;
    DeviceGuard guard(ix->device);
    DevPtr<unsigned int> d_hist;  // (one allocation for both passes over the words)
    HIP_TRY(d_hist.alloc(256));
    // one pass: the device histogram cleared, `launch` on the NULL stream, `bytes` of it copied back (which waits for it)
    auto pass = [&](void *host, size_t bytes, auto launch) {
        hipError_t err = hipMemsetAsync(d_hist, 0, bytes, nullptr);
        if (err == hipSuccess) {
            launch();
            err = hipGetLastError();
        }
        return err == hipSuccess ? hipMemcpy(host, d_hist, bytes, hipMemcpyDeviceToHost) : err;
    };
    const int shift = ix->packed_fmt == 12 ? 0 : 16;
    hipError_t err;
    if (dense_only) {
        const uint64_t blocks = (groups + 255) / 256, step = blocks / 4096 + 1, grid = (blocks + step - 1) / step;
        err = pass(ix->len_hist, sizeof(ix->len_hist), [&] {
            hipLaunchKernelGGL(dense_census_kernel, dim3((unsigned)grid), dim3(256), 0, nullptr, reinterpret_cast<const uint4 *>(ix->p3.p),
                               drows, step, d_hist);
        });
    } else {
        const uint64_t blocks = (ix->rows + 1023) / 1024, step = blocks / 4096 + 1, grid = (blocks + step - 1) / step;
        err = pass(ix->len_hist, sizeof(ix->len_hist), [&] {
            hipLaunchKernelGGL(len_census_kernel, dim3((unsigned)grid), dim3(256), 0, nullptr, ix->pk, ix->rows, shift, step, d_hist);
        });
        // ... and, exactly, WHICH overlaps occur (every row, not a sample): the sweeps for k - 1 >= 64 allocate, clear and fold
        // only the level arrays some row of the index can write to (memo_sweep_cons.hip: level_plan)
        if (err == hipSuccess)
            err = pass(ix->len_seen, sizeof(ix->len_seen), [&] {
                hipLaunchKernelGGL(len_seen_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, nullptr, ix->pk, ix->rows,
                                   shift, d_hist);
            });
    }
    if (err != hipSuccess) return fail(MEMO_EHIP, "overlap census: %s", hipGetErrorString(err));
    for (unsigned int c : ix->len_hist) ix->len_hist_rows += c;
    // (the dense rows' histogram: when rows that never write were left out of them, scale it to the index's rows so
    // that shares are shares of ix->rows, as they are for an index with 4-byte rows)
    if (dense_only && ix->boff3 && ix->len_hist_rows) {
        const double gone = (double)(ix->rows - ix->rows3) / (double)ix->rows3;
        ix->len_hist[255] += (unsigned int)(gone * (double)ix->len_hist_rows);
        ix->len_hist_rows += (unsigned int)(gone * (double)ix->len_hist_rows);
    }
    ix->len_seen_exact = dense_only ? 0 : 1;
    return MEMO_OK;
}

extern "C" {

const char *memo_last_error(void) { return g_err; }

const char *memo_version(void) { return "memo_amd 0.1 (gfx950)"; }

int memo_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int memo_index_create(uint64_t rows, int32_t device, memo_index_t **out) {
    if (!out) return fail(MEMO_EINVAL, "out is NULL");
    *out = nullptr;
    if (rows > ((uint64_t)1 << 40)) return fail(MEMO_EINVAL, "too many rows");
    memo_index *ix = nullptr;
    if (int rc = new_index(rows, device, nullptr, &ix)) return rc;
    DeviceGuard guard(device);
    const uint64_t padded = ix->padded;
    hipError_t err = ix->s.alloc(padded);
    if (err == hipSuccess) err = ix->e.alloc(padded);
    if (err == hipSuccess) err = ix->o.alloc(padded);
    if (err != hipSuccess) {
        memo_index_destroy(ix);
        return fail(MEMO_EHIP, "hipMalloc of %zu bytes x3 failed: %s", (size_t)padded * sizeof(int64_t), hipGetErrorString(err));
    }
    *out = ix;
    return MEMO_OK;
}

void memo_index_destroy(memo_index_t *ix) {
    if (!ix) return;
    DeviceGuard guard(ix->device);
    rows_changed(ix, kLevelColumns);  // (views and tile tables have no owner of their own)
    ix->d_status.reset();             // (every index has one: this hipFree is what waits for the device before the retire list goes)
    flush_retired(ix);
    delete ix;
}

int memo_index_upload(memo_index_t *ix, const int64_t *start, const int64_t *end,
                      const int64_t *annot, uint64_t rows) {
    if (!ix) return fail(MEMO_EINVAL, "index is NULL");
    if (rows != ix->rows) return fail(MEMO_EINVAL, "upload of %llu rows into an index of %llu",
                                      (unsigned long long)rows, (unsigned long long)ix->rows);
    return memo_index_upload_rows(ix, 0, start, end, annot, rows);
}

int memo_index_upload_rows(memo_index_t *ix, uint64_t row_offset, const int64_t *start,
                           const int64_t *end, const int64_t *annot, uint64_t rows) {
    if (!ix) return fail(MEMO_EINVAL, "index is NULL");
    if (row_offset > ix->rows || rows > ix->rows - row_offset)
        return fail(MEMO_EINVAL, "rows [%llu, +%llu) do not fit an index of %llu rows",
                    (unsigned long long)row_offset, (unsigned long long)rows, (unsigned long long)ix->rows);
    if (rows && (!start || !end || !annot)) return fail(MEMO_EINVAL, "column pointer is NULL");
    if (int rc = need_wide(ix)) return rc;
    DeviceGuard guard(ix->device);
    rows_changed(ix, kLevelColumns);
    if (rows) {
        HIP_TRY(hipMemcpy(ix->s + row_offset, start, rows * sizeof(int64_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(ix->e + row_offset, end, rows * sizeof(int64_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(ix->o + row_offset, annot, rows * sizeof(int64_t), hipMemcpyHostToDevice));
    }
    return MEMO_OK;
}

int memo_index_truncate(memo_index_t *ix, uint64_t rows) {
    if (!ix) return fail(MEMO_EINVAL, "index is NULL");
    if (rows > ix->rows) return fail(MEMO_EINVAL, "cannot grow an index (%llu > %llu rows)",
                                     (unsigned long long)rows, (unsigned long long)ix->rows);
    if (int rc = need_wide(ix)) return rc;
    DeviceGuard guard(ix->device);
    rows_changed(ix, kLevelColumns);
    ix->rows = rows;  // `padded` keeps the allocated size; finalize() rewrites the sentinel rows behind `rows`
    return MEMO_OK;
}

int memo_index_columns(memo_index_t *ix, int64_t **d_start, int64_t **d_end, int64_t **d_annot) {
    if (!ix) return fail(MEMO_EINVAL, "index is NULL");
    if (int rc = need_wide(ix)) return rc;
    DeviceGuard guard(ix->device);
    rows_changed(ix, kLevelColumns);  // (it only hands out pointers, but the caller may be about to rewrite the rows through them)
    if (d_start) *d_start = ix->s;
    if (d_end) *d_end = ix->e;
    if (d_annot) *d_annot = ix->o;
    return MEMO_OK;
}

int memo_index_finalize(memo_index_t *ix, int32_t bucket_shift, int32_t allow_sort) {
    if (!ix) return fail(MEMO_EINVAL, "index is NULL");
    if (int rc = need_wide(ix)) return rc;
    if (bucket_shift <= 0) bucket_shift = kDefaultBucketShift;
    if (bucket_shift > 8) return fail(MEMO_EINVAL, "bucket_shift must be <= 8 (tile width 256)");
    DeviceGuard guard(ix->device);
    hipStream_t st = nullptr;
    const uint64_t rows = ix->rows;
    // (the pk / pa allocations stay: a device sort below leaves the words stale, and the pack that follows reuses them)
    rows_changed(ix, kLevelColumns, true);
    {
        const uint64_t npad = ix->padded - rows;
        hipLaunchKernelGGL(pad_rows_kernel, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, st,
                           ix->s, ix->e, ix->o, rows, ix->padded);
        HIP_TRY(hipGetLastError());
    }
    uint64_t h[8] = {0};
    ix->was_sorted = 1;
    if (rows) {
        HIP_TRY(hipMemsetAsync(ix->d_scratch, 0, 64, st));
        const unsigned grid = (unsigned)(rows / 256 + 1 < 4096 ? rows / 256 + 1 : 4096);
        hipLaunchKernelGGL(check_rows_kernel, dim3(grid), dim3(256), 0, st, ix->s, ix->e, rows,
                           ix->d_scratch);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(h, ix->d_scratch, 24, hipMemcpyDeviceToHost));
        if (h[2]) return fail(MEMO_EINVAL, "%llu rows have coordinates beyond +-2^61", (unsigned long long)h[2]);
        if (int rc = ix->long_rows.collect(ix, h[1], st)) return rc;  // rows with end < start: set aside for long_rows_kernel
        if (h[0]) {
            ix->was_sorted = 0;
            if (!allow_sort)
                return fail(MEMO_EUNSORTED, "rows are not sorted by start (%llu descents)",
                            (unsigned long long)h[0]);
            char msg[256] = "";
            if (memo_sort_rows_by_start(ix->s, ix->e, ix->o, rows, ix->padded, st, msg, sizeof msg) != 0)
                return fail(MEMO_EHIP, "device sort failed: %s", msg);
        }
        HIP_TRY(hipMemcpy(&ix->min_s, ix->s, sizeof(int64_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&ix->max_s, ix->s + (rows - 1), sizeof(int64_t), hipMemcpyDeviceToHost));
    } else {
        ix->min_s = 0;
        ix->max_s = -1;
    }
    // buckets 0 .. ceil((max_s + 1) / width), plus one pinned to `rows`
    const int64_t top = ix->max_s < 0 ? 0 : ix->max_s;
    const uint64_t nb = (uint64_t)((top >> bucket_shift) + 3);
    HIP_TRY(ix->boff.alloc(nb));
    hipLaunchKernelGGL(bucket_table_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st,
                       ix->s, rows, ix->boff, nb, bucket_shift);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    ix->nb = nb;
    ix->bshift = bucket_shift;
    ix->finalized = 1;
    return MEMO_OK;
}

int memo_index_pack(memo_index_t *ix, int32_t keep_wide) {
    if (!ix) return fail(MEMO_EINVAL, "index is NULL");
    if (!ix->finalized) return fail(MEMO_ENOTREADY, "index not finalized");
    if (!ix->has_wide) {  // packed already (a builder's or an imported index): bring its rows into the query order now
        if (!ix->packed_fmt) return fail(MEMO_EINVAL, "nothing to pack");
        return ix->order_pending ? order_words_now(ix, row_order_mode(ix)) : MEMO_OK;
    }
    if (ix->rows && ix->min_s < 0) return fail(MEMO_EINVAL, "rows with a negative start cannot be packed");
    DeviceGuard guard(ix->device);
    hipStream_t st = nullptr;
    // (words of the same size are reused -- packing again after a re-finalize, or to time the pass; pa stays with them until the
    // layout is known)
    rows_changed(ix, kLevelWords, ix->pk && ix->packed_rows == ix->padded);
    if (!ix->pk) HIP_TRY(ix->pk.alloc(ix->padded));
    ix->packed_rows = ix->padded;
    uint64_t h[8] = {0};
    int fmt = 4;
    // The pass is timed on the device (info.pack_ms): SURVEY.md 8(d) wants the narrowing pass reported apart from the query.
    // Between the events: the census, the packing kernel and the order inside the buckets; the words' allocation is outside.
    float ms = 0.f;
    const int rc = build_timed(st, &ms, [&]() -> int {
        // The layout follows from the largest annot: guessed from a sample of the annot column (every 256th row), packed at once with
        // the exact census taken on the way, packed again only when a row the sample missed needs a wider layout.
        auto layout_of = [](uint64_t top) { return top <= 255 ? 4 : (top <= 4095 ? 12 : 6); };
        if (ix->rows) {
            HIP_TRY(hipMemsetAsync(ix->d_scratch, 0, 64, st));
            // (~2.6 * 10^5 samples: each is a cache line of its own from a step of 16 on, and every 256th row took 0.21 ms on 5 * 10^8 rows)
            const uint64_t step = ix->rows > (1u << 20) ? (ix->rows >> 18 > 256 ? ix->rows >> 18 : 256) : 1, samples = ix->rows / step + 1;
            const unsigned grid = (unsigned)(samples / 256 + 1 < 4096 ? samples / 256 + 1 : 4096);
            hipLaunchKernelGGL(annot_census_kernel, dim3(grid), dim3(256), 0, st, ix->o, ix->rows, ix->d_scratch, step);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpy(h, ix->d_scratch, 64, hipMemcpyDeviceToHost));
            if (h[3])  // (the index is left with packed_fmt == 0 and its buffers)
                return fail(MEMO_EINVAL, "rows have an annot outside [0, 65535]: cannot be packed");
            fmt = layout_of(h[5]);
            for (int pass = 0; pass < 2; ++pass) {
                if (fmt == 6 && !ix->pa) HIP_TRY(ix->pa.alloc(ix->padded));
                HIP_TRY(hipMemsetAsync(ix->d_scratch, 0, 64, st));
                hipLaunchKernelGGL(pack_rows_kernel, dim3(4096), dim3(256), 0, st, ix->s, ix->e, ix->o, ix->rows, ix->padded, ix->pk,
                                   fmt == 6 ? ix->pa.p : nullptr, fmt, pass == 0 ? ix->d_scratch.p : nullptr);
                HIP_TRY(hipGetLastError());
                if (pass) break;
                HIP_TRY(hipMemcpyAsync(h, ix->d_scratch, 64, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
                if (h[3])
                    return fail(MEMO_EINVAL, "%llu rows have an annot outside [0, 65535]: cannot be packed", (unsigned long long)h[3]);
                if (layout_of(h[5]) == fmt) break;
                fmt = layout_of(h[5]);  // (a row the sample missed: once more, in the layout it needs)
            }
        } else {
            hipLaunchKernelGGL(pack_rows_kernel, dim3(64), dim3(256), 0, st, ix->s, ix->e, ix->o, ix->rows, ix->padded, ix->pk, nullptr, fmt,
                               nullptr);
            HIP_TRY(hipGetLastError());
        }
        ix->max_annot = h[5];
        if (fmt != 6) ix->pa.reset();  // (only format 6 has the annot column)
        ix->row_order = 0;
        int mode = row_order_mode(ix);
        if (mode == 3 && ix->bshift != 5) mode = 2;  // (what interleave_words makes of it, and order_words_now records)
        if (mode && (fmt == 4 || fmt == 12) && ix->rows) {  // the order inside a bucket (memo_interleave.hip)
            if (int r = interleave_words(ix->pk, ix->boff, ix->nb, ix->bshift, fmt, mode, st, ix->d_scratch)) return r;
            ix->row_order = mode;
        }
        return MEMO_OK;
    });
    if (rc) return rc;
    ix->pack_ms = ms;
    ix->packed_fmt = fmt;
    if (int rc2 = memo_len_census(ix)) return rc2;
    if (!keep_wide) {
        ix->s.reset();
        ix->e.reset();
        ix->o.reset();
        ix->has_wide = 0;
    }
    return MEMO_OK;
}

int memo_index_pack_dense(memo_index_t *ix, int32_t keep_packed) {
    if (!ix) return fail(MEMO_EINVAL, "index is NULL");
    if (!ix->finalized) return fail(MEMO_ENOTREADY, "index not finalized");
    DeviceGuard guard(ix->device);
    if (!ix->p3) {
        if (!ix->pk || (ix->packed_fmt != 4 && !(ix->packed_fmt == 12 && ix->max_annot <= 511)))
            return fail(MEMO_EINVAL, "dense rows are built from the 4-byte rows: memo_index_pack first, and every annot <= 511");
        hipStream_t st = nullptr;
        const uint64_t groups = dense_groups_for(ix->padded);
        HIP_TRY(ix->p3.alloc(groups * 4));
        hipLaunchKernelGGL(pack3_rows_kernel, dim3(4096), dim3(256), 0, st, ix->pk, ix->padded, groups,
                           reinterpret_cast<uint4 *>(ix->p3.p), ix->packed_fmt == 12 ? 1 : 0);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
        ix->rows3 = ix->rows;
        ix->padded3 = ix->padded;
        if (int rc = dense_compact(ix)) return rc;
    }
    // Not a change of the rows: they stay what they are, and one copy of them leaves with its views.  packed_fmt stays as it is -- the
    // state a dense builder produces; on an index that had its dense rows already this is all the call does.
    if (!keep_packed && ix->pk) {
        drop_packed_views(ix);
        ix->pk.reset();
        ix->packed_rows = 0;
    }
    return MEMO_OK;
}

static void fill_info(const memo_index *ix, memo_index_info_t *info) {
    memset(info, 0, sizeof *info);
    info->version = MEMO_INDEX_INFO_VERSION;
    info->rows = ix->rows;
    info->min_start = ix->min_s;
    info->max_start = ix->max_s;
    info->device = ix->device;
    info->bucket_shift = ix->bshift;
    info->buckets = ix->nb;
    info->was_sorted = ix->was_sorted;
    info->finalized = ix->finalized;
    info->packed_format = ix->packed_fmt;
    info->has_wide = ix->has_wide;
    info->pack_ms = ix->pack_ms;
    info->last_sweep = ix->last_sweep;
    info->last_variant = ix->last_variant;
    info->dense_rows = ix->p3 ? 1 : 0;
    info->long_rows = ix->long_rows.n;
    info->max_annot = ix->max_annot;
    info->bucket_base = ix->bbase;
    info->device_bytes = (ix->has_wide ? ix->padded * 3 * sizeof(int64_t) : 0) + ix->nb * sizeof(int64_t) + 128 +
                         (ix->pk ? ix->padded * 4 : 0) + (ix->pa ? ix->padded * 2 : 0) +
                         (ix->p3 ? dense_groups_for(ix->boff3 ? ix->padded3 : ix->padded) * 16 : 0) + (ix->boff3 ? ix->nb * 8 : 0);
    info->dense_row_count = ix->p3 ? (ix->boff3 ? ix->rows3 : ix->rows) : 0;
    info->last_rows_read = ix->last_rows_read;
    info->last_view_ms = ix->last_view_ms;
    info->row_order = ix->row_order;
    uint64_t side = ix->retired_bytes;
    for (bool dense : {true, false})
        each_view(ix, dense, [&](const memo_index::DenseView &v) {
            side += v.p3 ? v.bytes + ix->nb * 8 : 0;
            side += v.dec.p3 ? v.dec_bytes + ix->nb * 8 : 0;  // (the deciding copy beside a live copy: side bytes, not a view of its own)
            side += v.run_bytes;                              // (... and the run copy beside that)
            info->views_resident += v.p3 ? 1 : 0;
        });
    for (const memo_index::TileTable &t : ix->ttabs) side += (uint64_t)t.n * 32;
    info->tile_tables_resident = (int32_t)ix->ttabs.size();
    info->side_bytes = side;
    info->device_bytes += side;
    info->view_builds = ix->view_builds;
    info->last_level_arrays = ix->last_arrays;
    info->view_placings = ix->view_placings;
    info->last_view_placed = ix->last_view_placed;
    info->last_view_rows_per_group = ix->last_view_rpg;
    info->last_tile_width = ix->last_tile_w;
}

int memo_index_get_info_v5(const memo_index_t *ix, memo_index_info_t *info) {
    if (!ix || !info) return fail(MEMO_EINVAL, "NULL argument");
    const uint32_t have = info->struct_bytes;
    if (have < 16)
        return fail(MEMO_EINVAL, "memo_index_info_t.struct_bytes = %u: set it to sizeof(memo_index_info_t) before the call", have);
    memo_index_info_t full;
    fill_info(ix, &full);
    // whole leading fields only: a size that ends inside a field is rounded down to where that field begins
#define MEMO_INFO_FIELD(f) (uint32_t) offsetof(memo_index_info_t, f)
    static const uint32_t starts[] = {
        MEMO_INFO_FIELD(struct_bytes), MEMO_INFO_FIELD(version), MEMO_INFO_FIELD(rows), MEMO_INFO_FIELD(min_start), MEMO_INFO_FIELD(max_start),
        MEMO_INFO_FIELD(device), MEMO_INFO_FIELD(bucket_shift), MEMO_INFO_FIELD(buckets), MEMO_INFO_FIELD(was_sorted), MEMO_INFO_FIELD(finalized),
        MEMO_INFO_FIELD(device_bytes), MEMO_INFO_FIELD(packed_format), MEMO_INFO_FIELD(has_wide), MEMO_INFO_FIELD(pack_ms), MEMO_INFO_FIELD(dense_rows),
        MEMO_INFO_FIELD(long_rows), MEMO_INFO_FIELD(max_annot), MEMO_INFO_FIELD(bucket_base), MEMO_INFO_FIELD(last_sweep), MEMO_INFO_FIELD(last_variant),
        MEMO_INFO_FIELD(dense_row_count), MEMO_INFO_FIELD(last_rows_read), MEMO_INFO_FIELD(last_view_ms), MEMO_INFO_FIELD(row_order),
        MEMO_INFO_FIELD(side_bytes), MEMO_INFO_FIELD(views_resident), MEMO_INFO_FIELD(tile_tables_resident), MEMO_INFO_FIELD(view_builds),
        MEMO_INFO_FIELD(last_level_arrays), MEMO_INFO_FIELD(last_view_placed), MEMO_INFO_FIELD(view_placings),
        MEMO_INFO_FIELD(last_view_rows_per_group), MEMO_INFO_FIELD(last_tile_width), (uint32_t)sizeof(memo_index_info_t)};
#undef MEMO_INFO_FIELD
    uint32_t n = 0;
    for (uint32_t s : starts)
        if (s <= have && s > n) n = s;
    full.struct_bytes = n;
    memcpy(info, &full, n);
    return MEMO_OK;
}


// {option, the field it sets, the values it takes: `lo`, and `first` .. `hi`, the refusal of any other}
static const struct {
    int32_t option;
    int memo_index::*field;
    int64_t lo, first, hi;
    const char *takes;
} kOptions[] = {
    {MEMO_OPT_VIEWS, &memo_index::views_on, 0, 1, 1, "MEMO_OPT_VIEWS takes 0 or 1"},
    {MEMO_OPT_VIEW_BUDGET_PCT, &memo_index::view_budget_pct, 0, 1, 1600, "MEMO_OPT_VIEW_BUDGET_PCT takes 0 .. 1600"},
    {MEMO_OPT_BUILD_COST_PCT, &memo_index::build_cost_pct, 0, 1, 100000, "MEMO_OPT_BUILD_COST_PCT takes 0 .. 100000"},
    {MEMO_OPT_VIEW_PLACES, &memo_index::view_places, 0, 1, 1, "MEMO_OPT_VIEW_PLACES takes 0 or 1"},
    {MEMO_OPT_VIEW_LIVE, &memo_index::view_live, 0, 1, 1, "MEMO_OPT_VIEW_LIVE takes 0 or 1"},  // (a copy already made stays: it answers exactly what the flagged view does)
    {MEMO_OPT_WIDE_TILES, &memo_index::wide_tiles, 0, 1, 1, "MEMO_OPT_WIDE_TILES takes 0 or 1"},
    {MEMO_OPT_VIEW_DECIDING, &memo_index::view_deciding, 0, 1, 1, "MEMO_OPT_VIEW_DECIDING takes 0 or 1"},  // (a copy already made stays, unread while the option is 0)
    {MEMO_OPT_VIEW_RUNS, &memo_index::view_runs, 0, 1, 1, "MEMO_OPT_VIEW_RUNS takes 0 or 1"},  // (a copy already made stays, unread while the option is 0)
    {MEMO_OPT_VIEW_ROWS, &memo_index::view_rows, 0, 5, 6, "MEMO_OPT_VIEW_ROWS takes 0 (the library's choice), 5 or 6"},
};

int memo_index_set_option(memo_index_t *ix, int32_t option, int64_t value) {
    if (!ix) return fail(MEMO_EINVAL, "index is NULL");
    for (const auto &o : kOptions) {
        if (o.option != option) continue;
        if (value != o.lo && (value < o.first || value > o.hi)) return fail(MEMO_EINVAL, "%s", o.takes);
        const int before = ix->*o.field;
        ix->*o.field = (int)value;
        // (the run copies want a host that has settled -- memo_view.hip, run_rows: one that changes, between its queries, which rows or
        // which kernel answer them has not; the budget and the cost share change neither)
        if (option != MEMO_OPT_VIEW_BUDGET_PCT && option != MEMO_OPT_BUILD_COST_PCT)
            for (memo_index::DenseView &v : ix->views6) v.run_answered = 0;
        if (option == MEMO_OPT_VIEWS && !value) {
            DeviceGuard guard(ix->device);
            HIP_TRY(hipDeviceSynchronize());
            // (the device is drained: the views are freed, not retired, and what drop_dense_views retires -- the tile tables made for
            // them -- is freed at once; the tables of the dense rows themselves stay)
            rows_changed(ix, kLevelDerived);
            flush_retired(ix);
        }
        return before;
    }
    return fail(MEMO_EINVAL, "unknown index option %d", option);
}

int memo_index_prepare(memo_index_t *ix, int32_t k, int32_t num_docs, int32_t membership, int64_t window_hint, void *stream,
                       uint64_t *bytes_taken) {
    if (bytes_taken) *bytes_taken = 0;
    if (!ix) return fail(MEMO_EINVAL, "index is NULL");
    if (!ix->finalized) return fail(MEMO_ENOTREADY, "index not finalized");
    if (window_hint < 0) return fail(MEMO_EINVAL, "window_hint must be >= 0");
    if (k <= 1 || !ix->rows) return MEMO_OK;  // (no row can write: nothing to build)
    DeviceGuard guard(ix->device);
    memo_index_info_t before, after;
    fill_info(ix, &before);
    // the window the queries to come are like: it starts on every kernel's tile grid, and nothing is ever written to d_out
    const int64_t top = ix->max_s < 0 ? 0 : ix->max_s;
    const int64_t len = window_hint > 0 ? window_hint : (top + 1 > 4096 ? top + 1 : 4096);
    void *const never_written = kNeverWritten;
    int rc;
    {
        struct PlanOnly {  // (the query path plans and builds, and launches nothing: reset on every way out of this scope)
            PlanOnly() { g_prepare_only = true; }
            ~PlanOnly() { g_prepare_only = false; }
        } plan_only;
        try {
            rc = membership ? memo_query_membership_dev(ix, 0, len, k, num_docs, static_cast<uint32_t *>(never_written), stream)
                 : num_docs <= 255 ? memo_query_conservation_u8_dev(ix, 0, len, k, num_docs, static_cast<uint8_t *>(never_written), stream)
                                   : memo_query_conservation_dev(ix, 0, len, k, num_docs, static_cast<uint16_t *>(never_written), stream);
        } catch (const std::exception &ex) {  // (the query path's std::vector / std::map may throw: no exception crosses the C ABI)
            rc = fail(MEMO_EHIP, "memo_index_prepare: %s", ex.what());
        }
    }
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());  // (views and tables are complete; and what the builds took out of service can go)
    flush_retired(ix);
    fill_info(ix, &after);
    if (bytes_taken) *bytes_taken = after.device_bytes > before.device_bytes ? after.device_bytes - before.device_bytes : 0;
    return MEMO_OK;
}

int memo_synth_fill(memo_index_t *ix, uint64_t row_begin, uint64_t num, uint64_t den,
                    int32_t num_docs, uint64_t seed) {
    if (!ix) return fail(MEMO_EINVAL, "index is NULL");
    if (num == 0 || den == 0 || num_docs < 2) return fail(MEMO_EINVAL, "bad generator parameters");
    if (int rc = need_wide(ix)) return rc;
    DeviceGuard guard(ix->device);
    rows_changed(ix, kLevelColumns);
    if (ix->rows) {
        hipLaunchKernelGGL(synth_rows_kernel, dim3(4096), dim3(256), 0, nullptr, ix->s, ix->e, ix->o,
                           ix->rows, row_begin, num, den, (uint64_t)(num_docs - 1), seed);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
    }
    return MEMO_OK;
}

int memo_bin_conservation_dev(const uint16_t *d_vec, int64_t L, const int64_t *edges, int32_t nbins,
                              int32_t num_docs, uint64_t *counts, int32_t device, void *stream) {
    if (nbins < 1 || num_docs < 1 || num_docs > 65534 || !edges || !counts || (L > 0 && !d_vec))
        return fail(MEMO_EINVAL, "bad binning arguments");
    for (int i = 0; i < nbins; ++i)
        if (edges[i] < 0 || edges[i] > edges[i + 1] || edges[i + 1] > L)
            return fail(MEMO_EINVAL, "bin edges must be non-decreasing inside [0, L]");
    OnDevice on(device, OnDevice::kSelectOnly);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int ncols = num_docs + 1;
    const size_t cbytes = (size_t)nbins * ncols * sizeof(uint64_t);
    const size_t ebytes = ((size_t)(nbins + 1) * sizeof(int64_t) + 15) & ~(size_t)15;
    // edges + counts live in one scratch buffer per (thread, device) that only ever grows: `memo view`
    // bins the same vector at several resolutions, and a hipMalloc / hipFree pair per call costs more
    // than the histogram
    struct Scratch {
        char *p = nullptr;
        size_t cap = 0;
        int dev = -1;  // (never freed at thread exit: the HIP runtime may be gone by then)
    };
    thread_local Scratch scratch;
    if (scratch.dev != device || scratch.cap < ebytes + cbytes) {
        if (scratch.p) (void)hipFree(scratch.p);
        scratch.p = nullptr;
        scratch.cap = 0;
        const size_t want = ebytes + cbytes < (1u << 20) ? (1u << 20) : ebytes + cbytes;
        hipError_t err = hipMalloc(&scratch.p, want);
        if (err != hipSuccess) return fail(MEMO_EHIP, "hipMalloc(%zu): %s", want, hipGetErrorString(err));
        scratch.cap = want;
        scratch.dev = device;
    }
    int64_t *d_edges = reinterpret_cast<int64_t *>(scratch.p);
    unsigned long long *d_counts = reinterpret_cast<unsigned long long *>(scratch.p + ebytes);
    hipError_t err = hipMemcpyAsync(d_edges, edges, (size_t)(nbins + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st);
    if (err == hipSuccess) err = hipMemsetAsync(d_counts, 0, cbytes, st);
    if (err == hipSuccess) {
        // enough workgroups to fill the chip, at least one per bin
        int slices = (int)((2048 + nbins - 1) / nbins);
        const int64_t longest = (L + nbins - 1) / nbins;
        while (slices > 1 && longest / slices < 4096) --slices;
        if ((size_t)ncols * 4 <= 48 * 1024)
            hipLaunchKernelGGL(bin_conservation_kernel<true>, dim3((unsigned)(nbins * slices)), dim3(256),
                               (size_t)ncols * 4, st, d_vec, d_edges, ncols, slices, d_counts);
        else
            hipLaunchKernelGGL(bin_conservation_kernel<false>, dim3((unsigned)(nbins * slices)), dim3(256), 0, st,
                               d_vec, d_edges, ncols, slices, d_counts);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipMemcpyAsync(counts, d_counts, cbytes, hipMemcpyDeviceToHost, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    if (err != hipSuccess) return fail(MEMO_EHIP, "binning failed: %s", hipGetErrorString(err));
    return MEMO_OK;
}

// ---- raw device buffers for hosts that do not bring their own allocator ---------------------
int memo_dev_malloc(int32_t device, size_t bytes, void **out) {
    if (!out) return fail(MEMO_EINVAL, "out is NULL");
    *out = nullptr;
    OnDevice on(device, OnDevice::kSelectOnly);
    if (on.rc) return on.rc;
    HIP_TRY(hipMalloc(out, bytes ? bytes : 16));
    return MEMO_OK;
}

int memo_dev_free(int32_t device, void *p) {
    DeviceGuard guard(device);
    HIP_TRY(hipFree(p));
    return MEMO_OK;
}

int memo_dev_upload(int32_t device, void *dev, const void *host, size_t bytes, void *stream) {
    DeviceGuard guard(device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (bytes) HIP_TRY(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MEMO_OK;
}

// large pageable host memory (a memory-mapped file): in pieces through the pinned ring
int memo_dev_upload_pipelined(int32_t device, void *dev, const void *host, size_t bytes) {
    if (bytes && (!dev || !host)) return fail(MEMO_EINVAL, "NULL buffer");
    if (int rc = device_ok(device)) return rc;
    return upload_pipelined(device, dev, host, bytes);
}

int memo_dev_download(int32_t device, void *host, const void *dev, size_t bytes, void *stream) {
    DeviceGuard guard(device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (bytes) HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MEMO_OK;
}

}  // extern "C"
