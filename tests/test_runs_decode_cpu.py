"""The lane decode of the run copy (memo_amd/csrc/memo_runs_decode.h) on the host: the same arithmetic the decode kernel runs per lane
-- the byte index of the lane's first position, the P / 4 + 1 dwords it loads, a selector per quartet -- with the device's v_perm_b32
replaced by a byte loop that takes the same selector (and traps on a selector byte past 7).  A stand-alone program, built with the address
and undefined-behaviour sanitizers, compares it with a brute-force expansion that walks the mask bit by bit; the values buffer is
exactly value_bytes + P bytes long, the read bound the header states, so a read past the pad is the sanitizer's."""
import os
import subprocess

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

DECODE_MAIN = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "memo_runs_decode.h"

// a byte pattern that does not repeat within 251 bytes (37 and 251 are coprime), with 255 among them
static uint8_t pattern(uint32_t i) {
    const uint32_t v = (i * 37u + 11u) % 251u;
    return v == 7u ? 255u : (uint8_t)v;
}

template <int P>
static int one_bucket(uint32_t mask, uint32_t off) {
    // the bucket is the last of the copy: its values end the allocation but for the dword padding of its group and the pad of P bytes
    const uint32_t value_bytes = (off + (uint32_t)__builtin_popcount(mask) + 3u) & ~3u;
    const size_t bytes = (size_t)value_bytes + P;
    uint8_t *vals = (uint8_t *)malloc(bytes);                               // exactly: a read past the pad is AddressSanitizer's
    for (uint32_t i = 0; i < value_bytes; ++i) vals[i] = pattern(i);
    memset(vals + value_bytes, 0, P);
    uint8_t want[32];
    uint32_t j = off - 1u;
    for (int i = 0; i < 32; ++i) {                                           // brute force: bit by bit
        j += (mask >> i) & 1u;
        want[i] = vals[j];
    }
    int bad = 0;
    for (uint32_t r = 0; r + P <= 32 && !bad; r += P) {
        const memo::RunQuartets<P> got = memo::runs_lane_decode<P>(mask, off, r, reinterpret_cast<const uint32_t *>(vals));
        for (int i = 0; i < P; ++i) {
            const uint8_t g = (uint8_t)(got.q[i / 4] >> (8 * (i % 4)));
            if (g != want[r + i]) {
                printf("P=%d mask=%08x offset=%u r=%u position %d: got %u, want %u\n", P, mask, off, r, i, g, want[r + i]);
                bad = 1;
                break;
            }
        }
    }
    free(vals);
    return bad;
}

template <int P>
static int all_cases() {
    uint64_t n = 0;
    auto every_offset = [&](uint32_t mask) {
        // off and off + 36: every A & 3 at every lane start, near the buffer's first byte and away from it
        for (uint32_t off = 0; off < 4; ++off) {
            if (one_bucket<P>(mask, off) || one_bucket<P>(mask, off + 36u)) return 1;
            n += 2;
        }
        return 0;
    };
    if (every_offset(1u) || every_offset(0xFFFFFFFFu) || every_offset(0x55555555u) || every_offset(0xAAAAAAABu)) return 1;
    for (int i = 0; i < 32; ++i)
        if (every_offset(1u | (1u << i))) return 1;                          // a single start bit at each of the 32 places
    uint64_t s = 0x9E3779B97F4A7C15ull;                                      // a fixed seed
    for (int i = 0; i < 4000; ++i) {
        s ^= s << 13, s ^= s >> 7, s ^= s << 17;
        uint32_t m = (uint32_t)(s >> 16);
        if (i % 3 == 1) m &= (uint32_t)(s >> 40) | (uint32_t)(s << 3);       // sparser
        if (i % 3 == 2) m |= (uint32_t)(s >> 33);                            // denser
        if (every_offset(m | 1u)) return 1;
    }
    printf("P=%d: %llu buckets\n", P, (unsigned long long)n);
    return 0;
}

int main() {
    if (all_cases<8>() || all_cases<16>()) return 1;
    puts("ok");
    return 0;
}
"""


def test_lane_decode_against_brute_force_under_sanitizers(tmp_path):
    src = tmp_path / "decode_main.cpp"
    src.write_text(DECODE_MAIN)
    exe = str(tmp_path / "decode_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "memo_amd", "csrc"), str(src), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.endswith("ok\n"), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "P=8: 32288 buckets" in r.stdout and "P=16: 32288 buckets" in r.stdout, r.stdout
