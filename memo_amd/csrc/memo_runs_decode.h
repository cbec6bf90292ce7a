// memo_runs_decode.h -- what ONE LANE does with the run copy (memo_view_build.hip: run_view_copy): P consecutive positions of one bucket
// from the bucket's table entry and the values.  Host and device run the same arithmetic; only the byte pick differs (v_perm_b32 on the
// device, a byte loop with the same selector on the host), so a host program can check the selectors (tests/test_runs_decode_cpu.py).
//
// The lane's first position is r inside its bucket (a multiple of P; P divides 32, so a lane never leaves its bucket).  Its value is byte
// A = offset + popcount(mask bits 0 .. r) - 1 of the values; the P positions want bytes at non-decreasing indices A .. A + P - 1.  The lane
// loads the P / 4 + 1 dwords from the dword that holds A on -- dword-aligned addresses, never a byte-unaligned load -- and every quartet of
// positions picks its four bytes out of two neighbouring ones of them.
// READ BOUND: bytes [A & ~3, (A & ~3) + P + 4).  A is below the copy's value_bytes, a multiple of four, so a lane reads at most P bytes
// past value_bytes: the zeroed pad behind the values (run_view_copy) has to hold P bytes.
#ifndef MEMO_RUNS_DECODE_H
#define MEMO_RUNS_DECODE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define MEMO_RUNS_HD __host__ __device__ __forceinline__
#else
#define MEMO_RUNS_HD inline
#endif

namespace memo {

template <int P>
struct RunQuartets {
    uint32_t q[P / 4];  // quartet j: the value bytes of positions r + 4 j .. r + 4 j + 3, the first in the low byte
};
template <int P>
struct RunDwords {
    uint32_t d[P / 4 + 1];
};

// byte i of the result: byte sel_i of hi:lo (0 .. 3: lo, 4 .. 7: hi), sel_i = byte i of sel
MEMO_RUNS_HD uint32_t runs_pick(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t both = ((uint64_t)hi << 32) | lo;
    uint32_t out = 0;
    for (int i = 0; i < 4; ++i) {
        const uint32_t s = (sel >> (8 * i)) & 255u;
        if (s > 7u) __builtin_trap();  // (v_perm_b32 gives constants and sign bytes from 8 on: never a value)
        out |= (uint32_t)((both >> (8 * s)) & 255u) << (8 * i);
    }
    return out;
#endif
}

// x (0 .. 3) in every byte: one full-rate v_perm_b32 where the multiplication is a quarter-rate v_mul_lo_u32
MEMO_RUNS_HD uint32_t runs_spread(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(0u, x, 0u);
#else
    return x * 0x01010101u;
#endif
}

// the byte index of the value of position r of the bucket (mask: its start bits, bit 0 always set; offset: the byte of its first value)
MEMO_RUNS_HD uint32_t runs_lane_first(uint32_t mask, uint32_t offset, uint32_t r) {
    return offset + (uint32_t)__builtin_popcount(mask & ((2u << r) - 1u)) - 1u;
}

// the lane's own dwords of the values: see READ BOUND above
template <int P>
MEMO_RUNS_HD RunDwords<P> runs_lane_load(const uint32_t *vals, uint32_t A) {
    RunDwords<P> D;
    const uint32_t *src = vals + (A >> 2);
#pragma unroll
    for (int i = 0; i < P / 4 + 1; ++i) D.d[i] = src[i];
    return D;
}

// Quartet j begins at byte b = (A & 3) + the starts among positions r + 1 .. r + 4 j, at most 3 + 4 j: inside dwords b / 4 <= j and the
// next one.  Its selector: byte i = (b & 3) + the starts among the quartet's positions 1 .. i, at most 3 + 3.
template <int P>
MEMO_RUNS_HD RunQuartets<P> runs_lane_pick(uint32_t mask, uint32_t r, uint32_t A, const RunDwords<P> &D) {
    static_assert(P == 8 || P == 16, "positions a lane: whole quartets, a divisor of the bucket");
    const uint32_t next = mask >> (r + 1u);  // bit i: position r + 1 + i starts a run (r + 1 <= 32 - P + 1)
    RunQuartets<P> out;
#pragma unroll
    for (int j = 0; j < P / 4; ++j) {
        const uint32_t b = (A & 3u) + (j ? (uint32_t)__builtin_popcount(next & ((1u << (4 * j)) - 1u)) : 0u);
        const uint32_t w = b >> 2;
        uint32_t lo = D.d[0], hi = D.d[1];
#pragma unroll
        for (int i = 1; i <= j; ++i) {
            lo = w >= (uint32_t)i ? D.d[i] : lo;
            hi = w >= (uint32_t)i ? D.d[i + 1] : hi;
        }
        const uint32_t steps = (((next >> (4 * j)) & 7u) * 0x408100u) & 0x01010100u;  // the next three start bits, one to a byte
        uint32_t sel = runs_spread(b & 3u) + steps;
        sel += steps << 8;
        sel += (steps & 0x0100u) << 16;
        out.q[j] = runs_pick(hi, lo, sel);
    }
    return out;
}

// entry (mask, offset), first position r, values -> the P value bytes
template <int P>
MEMO_RUNS_HD RunQuartets<P> runs_lane_decode(uint32_t mask, uint32_t offset, uint32_t r, const uint32_t *vals) {
    const uint32_t A = runs_lane_first(mask, offset, r);
    return runs_lane_pick<P>(mask, r, A, runs_lane_load<P>(vals, A));
}

}  // namespace memo

#endif  // MEMO_RUNS_DECODE_H
