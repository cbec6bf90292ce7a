// memo_runs.hip -- `memo regions`: the maximal runs of equal key of a query result that is still in HBM, compacted there, so that
// intervals and not one line per position leave the device.  No counterpart in the reference (its users run-length the text of
// memo_query.py:65-71 on the host).
//
// A BOUNDARY is a position whose key differs from the key of the position before it.  Three keys:
//   value   key = vec[i]                       position 0 is a boundary; starts[r], values[r] per run: lossless
//   band    key = lo <= vec[i] && vec[i] <= hi the position before the window counts as false, so position 0 is a boundary iff its
//                                              key is true; only boundaries are stored: 2j opens an interval, 2j + 1 closes it, an
//                                              odd count leaves the last interval to end at L
//   bits    key = the W words of position i    position 0 is a boundary; starts[r] and the W words of the run per run.  Bits at or
//                                              above num_docs are 0 by the result encoding (include/memo_amd.h: result encodings): whole words compare
// Each is a key of memo_compact.h's compaction, on one plane.  A key owns kPer positions per lane and load: the 16 bytes a lane loads hold 8 uint16
// values, or 4 one-word rows, or 2 two-word rows (PackedKey: an element is an integer); any other W takes one row per lane, its
// words loaded 4, 2 or 1 at a time as W allows (RowKey: right for every W >= 1, rows of an odd W lie off the 16-byte grid).
//
// Three launches, ordered by the stream (memo_compact.h): the count per tile of 256 lanes x 4 loads x kPer positions, the scan of
// the tile counts, the scatter of starts[rank] = i and the key's payload.  The host reads the total between the scan and the scatter
// and allocates exactly that many entries.
//
// Conditions the code holds:
//   - no workgroup waits for another: no look-back, no flag in memory, no cooperative launch
//   - nothing is read before vec[0] or at or past vec[L] (vec[L * W]): a lane's first position is compared with the lane below
//     through a wave shuffle, a wave's first with one extra load of vec[i - 1] that is not made at i == 0; a load that would
//     cross L is made element by element for the elements before L
//   - d_vec is 16-byte aligned (anything else is MEMO_EINVAL before any launch)
//   - L == 0 launches nothing; L and positions are int64, tile counts uint32, bases and totals 64-bit
//   - a position at or past L never sets a flag, and the scatter writes no rank at or past the total
#include <type_traits>

#include "memo_compact.h"

using namespace memo;

namespace {

const int kNeverTimed = 0;  // (`memo regions` has no timed form: the compaction's laps stay off)

__device__ __forceinline__ uint32_t shfl_up1(uint32_t x) { return (uint32_t)__shfl_up((int)x, 1, 64); }
__device__ __forceinline__ uint64_t shfl_up1(uint64_t x) { return (uint64_t)__shfl_up((unsigned long long)x, 1, 64); }

// elements that are integers: E = uint16_t (conservation values), uint32_t / uint64_t (membership rows of one / two words)
template <typename E, bool kBand>
struct PackedKey {
    static constexpr int kPer = 16 / (int)sizeof(E);
    using K = typename std::conditional<(sizeof(E) > 4), uint64_t, uint32_t>::type;  // what is compared and shuffled
    using Start = int64_t;
    const E *vec;
    E *payload;  // values[] / run_bits[]; nullptr for a band
    int64_t L;
    uint32_t lo, hi;

    __device__ __forceinline__ void tile_of(int64_t block, int64_t &plane, int64_t &p0) const { plane = 0, p0 = block * tile_positions<PackedKey>(); }

    __device__ __forceinline__ K key(E v) const { return kBand ? (K)(lo <= (uint32_t)v && (uint32_t)v <= hi) : (K)v; }

    // bit j: position p + j (p a multiple of kPer) is a boundary.  Called by whole waves (it shuffles).
    __device__ __forceinline__ uint32_t flags(int64_t, int64_t p) const {
        E e[kPer];
        if (p + kPer <= L) {
            const uint4 q = *reinterpret_cast<const uint4 *>(vec + p);
            memcpy(e, &q, 16);
        } else {
#pragma unroll
            for (int j = 0; j < kPer; ++j) e[j] = p + j < L ? vec[p + j] : E(0);
        }
        K prev = shfl_up1(key(e[kPer - 1]));
        if ((threadIdx.x & 63) == 0 && p > 0 && p < L) prev = key(vec[p - 1]);
        if (p == 0) prev = kBand ? K(0) : ~key(e[0]);
        uint32_t m = 0;
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const K k = key(e[j]);
            m |= (uint32_t)(k != prev && p + j < L) << j;
            prev = k;
        }
        return m;
    }

    __device__ __forceinline__ void store(int64_t, int64_t rank, int64_t i) const {
        if (!kBand) payload[rank] = vec[i];
    }
};

// a row of W words per lane, V words per load (W a multiple of V)
template <int V>
struct RowKey {
    static constexpr int kPer = 1;
    using Vec = typename std::conditional<V == 4, uint4, typename std::conditional<V == 2, uint2, uint32_t>::type>::type;
    using Start = int64_t;
    const uint32_t *vec;
    uint32_t *payload;
    int64_t L;
    int W;

    __device__ __forceinline__ void tile_of(int64_t block, int64_t &plane, int64_t &p0) const { plane = 0, p0 = block * tile_positions<RowKey>(); }

    __device__ __forceinline__ uint32_t flags(int64_t, int64_t p) const {
        const bool valid = p < L, own_prev = (threadIdx.x & 63) == 0 && valid && p > 0;
        bool diff = false;
        for (int c = 0; c < W; c += V) {
            uint32_t x[V] = {};
            if (valid) {
                const Vec q = *reinterpret_cast<const Vec *>(vec + p * W + c);
                memcpy(x, &q, sizeof q);
            }
#pragma unroll
            for (int v = 0; v < V; ++v) {
                uint32_t px = shfl_up1(x[v]);  // (lane 0 gets its own word back: p == 0 is a boundary without it)
                if (own_prev) px = vec[(p - 1) * W + c + v];
                diff |= x[v] != px;
            }
        }
        return valid && (p == 0 || diff) ? 1u : 0u;
    }

    __device__ __forceinline__ void store(int64_t, int64_t rank, int64_t i) const {
        for (int c = 0; c < W; c += V)
            *reinterpret_cast<Vec *>(payload + rank * W + c) = *reinterpret_cast<const Vec *>(vec + i * W + c);
    }
};

// count, scan, allocate exactly, scatter.  payload_bytes: of one payload entry per run (0: none).  Blocking.
template <typename Key>
int compact_runs(Key key, size_t payload_bytes, int64_t **d_starts, void **d_payload, uint64_t *runs, hipStream_t st) {
    constexpr int64_t T = tile_positions<Key>();
    const int64_t ntiles = (key.L + T - 1) / T;
    if (ntiles > INT32_MAX) return fail(MEMO_EINVAL, "a result of %lld positions is too long", (long long)key.L);
    Compaction c(st, kNeverTimed, nullptr);
    HIP_TRY(c.lay_out(ntiles, 0));
    if (int rc = c.count(key)) return rc;
    const int64_t total = c.total();
    if (total <= 0) return MEMO_OK;
    DevPtr<int64_t> starts;
    DevPtr<char> payload;
    const size_t sbytes = (size_t)total * sizeof(int64_t), pbytes = (size_t)total * payload_bytes;
    if (hipError_t err = starts.alloc((size_t)total); err != hipSuccess)
        return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the starts of %lld runs: %s", sbytes, (long long)total, hipGetErrorString(err));
    if (pbytes)
        if (hipError_t err = payload.alloc(pbytes); err != hipSuccess)
            return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the values of %lld runs: %s", pbytes, (long long)total, hipGetErrorString(err));
    key.payload = reinterpret_cast<decltype(key.payload)>(payload.p);
    if (int rc = c.scatter(key, starts.p)) return rc;
    *runs = (uint64_t)total;
    *d_starts = starts.release();
    if (d_payload) *d_payload = payload.release();
    return MEMO_OK;
}

int check_vector(const void *d_vec, int64_t L) {
    if (L < 0 || (L && !d_vec)) return fail(MEMO_EINVAL, "bad result vector (L = %lld)", (long long)L);
    if (reinterpret_cast<uintptr_t>(d_vec) & 15) return fail(MEMO_EINVAL, "d_vec must be 16-byte aligned");
    return MEMO_OK;
}

}  // namespace

extern "C" {

int32_t memo_runs_tile(int32_t words) {
    if (words <= 0) return tile_positions<PackedKey<uint16_t, false>>();
    return words == 1 ? tile_positions<PackedKey<uint32_t, false>>()
                      : words == 2 ? tile_positions<PackedKey<uint64_t, false>>() : tile_positions<RowKey<1>>();
}

int memo_runs_conservation_dev(const uint16_t *d_vec, int64_t L, int32_t mode, int32_t lo, int32_t hi, int64_t **d_starts,
                               uint16_t **d_values, uint64_t *runs, int32_t device, void *stream) {
    if (!d_starts || !runs || (mode == 0 && !d_values)) return fail(MEMO_EINVAL, "d_starts / d_values / runs is NULL");
    *d_starts = nullptr;
    *runs = 0;
    if (d_values) *d_values = nullptr;
    if (mode != 0 && mode != 1) return fail(MEMO_EINVAL, "mode %d: 0 (value) or 1 (band)", mode);
    if (mode == 1 && (lo < 0 || hi > 65535 || lo > hi)) return fail(MEMO_EINVAL, "band [%d, %d]: 0 <= lo <= hi <= 65535", lo, hi);
    if (int rc = check_vector(d_vec, L)) return rc;
    if (!L) return MEMO_OK;
    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (mode == 1) return compact_runs(PackedKey<uint16_t, true>{d_vec, nullptr, L, (uint32_t)lo, (uint32_t)hi}, 0, d_starts, nullptr, runs, st);
    return compact_runs(PackedKey<uint16_t, false>{d_vec, nullptr, L, 0, 0}, sizeof(uint16_t), d_starts, reinterpret_cast<void **>(d_values),
                        runs, st);
}

int memo_runs_membership_dev(const uint32_t *d_bits, int64_t L, int32_t num_docs, int64_t **d_starts, uint32_t **d_run_bits,
                             uint64_t *runs, int32_t device, void *stream) {
    if (!d_starts || !runs || !d_run_bits) return fail(MEMO_EINVAL, "d_starts / d_run_bits / runs is NULL");
    *d_starts = nullptr;
    *d_run_bits = nullptr;
    *runs = 0;
    if (num_docs < 1) return fail(MEMO_EINVAL, "num_docs must be at least 1");
    if (int rc = check_vector(d_bits, L)) return rc;
    if (!L) return MEMO_OK;
    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int W = (num_docs + 31) / 32;
    void **out = reinterpret_cast<void **>(d_run_bits);
    const size_t row = (size_t)W * sizeof(uint32_t);
    if (W == 1) return compact_runs(PackedKey<uint32_t, false>{d_bits, nullptr, L, 0, 0}, row, d_starts, out, runs, st);
    if (W == 2)
        return compact_runs(PackedKey<uint64_t, false>{reinterpret_cast<const uint64_t *>(d_bits), nullptr, L, 0, 0}, row, d_starts, out, runs, st);
    if (W % 4 == 0) return compact_runs(RowKey<4>{d_bits, nullptr, L, W}, row, d_starts, out, runs, st);
    if (W % 2 == 0) return compact_runs(RowKey<2>{d_bits, nullptr, L, W}, row, d_starts, out, runs, st);
    return compact_runs(RowKey<1>{d_bits, nullptr, L, W}, row, d_starts, out, runs, st);
}

}  // extern "C"
