// memo_planes.h -- membership rows as per-genome bit planes: what memo_cooc.hip (`memo matrix`) and memo_collect.hip (`memo collect`)
// stage in LDS before they reduce over positions.  A 32 x 32 block of a membership result -- 32 consecutive rows of one genome word
// -- is transposed in registers, so that word j of the block holds 32 positions of genome 32 w + j.
// (transpose32 is memo_sweep_memb.hip's, copied: that file's generated code stays as it is.)
#ifndef MEMO_PLANES_H
#define MEMO_PLANES_H

#include "memo_common.h"

namespace memo {

constexpr int kPlaneBlockPitch = 36;  // LDS words from one staged genome word's 32 planes to the next: the lanes' 16-byte stores then
                                      // fall on all banks alike (a position word's row is 36 x staged words + 4)

template <int J>
__device__ __forceinline__ void transpose32_stage(uint32_t (&m)[32]) {
    constexpr uint32_t mask = J == 4 ? 0x0F0F0F0Fu : J == 2 ? 0x33333333u : 0x55555555u;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        if ((k & J) == 0) {
            const uint32_t a = m[k], b = m[k + J];
            if (J == 16) {
                m[k] = __builtin_amdgcn_perm(b, a, 0x05040100u);      // a.lo16 | b.lo16 << 16
                m[k + J] = __builtin_amdgcn_perm(b, a, 0x07060302u);  // a.hi16 | b.hi16 << 16
            } else if (J == 8) {
                m[k] = __builtin_amdgcn_perm(b, a, 0x06020400u);      // bytes a0 b0 a2 b2
                m[k + J] = __builtin_amdgcn_perm(b, a, 0x07030501u);  // bytes a1 b1 a3 b3
            } else {
                const uint32_t bs = b << J, as = a >> J;
                asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(m[k]) : "s"(mask), "v"(a), "v"(bs));
                asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(m[k + J]) : "s"(mask), "v"(as), "v"(b));
            }
        }
    }
}

__device__ __forceinline__ void transpose32(uint32_t (&m)[32]) {  // m[j] bit i  <-  m[i] bit j
    transpose32_stage<16>(m);
    transpose32_stage<8>(m);
    transpose32_stage<4>(m);
    transpose32_stage<2>(m);
    transpose32_stage<1>(m);
}

// One block into LDS: the rows r0 .. r0 + 31 of genome word w of a result bits[L][W] of N genomes, as 32 plane words at dst (16-byte
// aligned).  One load per row word, of the rows before L only: a row at or past L is staged as zeros, and so are the bits at or above
// N, whatever the rows hold.  (cooc_kernel keeps these lines inline: called from here its registers came out otherwise allocated,
// 78 / 117 VGPRs for 79 / 119, and that kernel's generated code stays the measured one.)
__device__ __forceinline__ void stage_plane_block(const uint32_t *bits, int64_t L, int W, int N, int w, int64_t r0, uint32_t *dst_words) {
    const uint32_t *src = bits + r0 * W + w;
    uint32_t m[32];
    if (r0 + 32 <= L) {
#pragma unroll
        for (int i = 0; i < 32; ++i) m[i] = src[(int64_t)i * W];
    } else {
#pragma unroll
        for (int i = 0; i < 32; ++i) m[i] = r0 + i < L ? src[(int64_t)i * W] : 0u;
    }
    const uint32_t below_n = (w == W - 1 && (N & 31)) ? (1u << (N & 31)) - 1u : 0xFFFFFFFFu;
#pragma unroll
    for (int i = 0; i < 32; ++i) m[i] &= below_n;
    transpose32(m);  // m[j]: genome 32 w + j, bit i: position r0 + i
    uint4 *dst = reinterpret_cast<uint4 *>(dst_words);
#pragma unroll
    for (int q = 0; q < 8; ++q) dst[q] = make_uint4(m[4 * q], m[4 * q + 1], m[4 * q + 2], m[4 * q + 3]);
}

}  // namespace memo

#endif  // MEMO_PLANES_H
