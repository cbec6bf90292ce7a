"""The worked tables of `memo cover` (README), shared by tests/test_cover_cpu.py (the oracle against them) and
tests/test_cover_gpu.py (the device against them).  Rows are (added, core, covered).  They were computed on the CPU by a NumPy
restatement of the definition (tests/cover_oracle.py) over tests/lengths_oracle.planes of the committed goldens."""

_A = [(3, 83, 83), (2, 72, 93), (4, 59, 94), (1, 49, 95)]

# example_memb.parquet, -n 5 -r ref_1:0-20: (flags of region_cover, L x span, rows)
EXAMPLE = [
    (dict(), 20 * (2 ** 31 - 1), _A),
    (dict(objective="core"), 20 * (2 ** 31 - 1), _A),
    (dict(kmax=8), 160, _A),
    (dict(kmax=8, objective="core"), 160, _A),
    (dict(kmin=3, kmax=8), 120, [(3, 43, 43), (2, 32, 53), (4, 19, 54), (1, 9, 55)]),
    (dict(kmin=3, kmax=3), 20, [(3, 20, 20), (4, 18, 20), (2, 16, 20), (1, 8, 20)]),            # `memo panel -k 3`
    (dict(kmin=4, kmax=4), 20, [(2, 12, 12), (3, 10, 14), (4, 3, 15), (1, 1, 16)]),             # `memo panel -k 4`, annot tie included
    (dict(kmin=5, kmax=5), 20, [(3, 8, 8), (2, 5, 10), (1, 0, 10), (4, 0, 10)]),
    (dict(kmax=8, candidates="1,2,4"), 160, [(2, 82, 82), (4, 61, 85), (1, 49, 88)]),
    (dict(kmax=8, seeds="1"), 160, [(1, 52, 52), (2, 49, 85), (3, 49, 94), (4, 49, 95)]),
    (dict(kmax=8, fraction="0.5"), 160, [(3, 83, 83)]),                                           # the threshold is 80
    (dict(kmax=8, fraction="0.6"), 160, _A),                                                      # the threshold of 96 is never reached
    (dict(kmax=8, max_genomes=2), 160, [(3, 83, 83), (2, 72, 93)]),
    (dict(kmax=8, seeds="4,1", fraction="0"), 160, [(4, 64, 64), (1, 49, 67)]),
]

# the first covered of single genomes at -K 8: `memo pairs -K 8`'s diagonal
EXAMPLE_DIAGONAL = {3: 83, 2: 82, 4: 64, 1: 52}

# rnd_n40.parquet, -n 40 -r chr1:0-2100: (flags, the order's first genomes, the first rows, the last row)
_K64 = [9, 3, 26, 7, 27, 35, 33, 25, 30, 38, 39, 21]
RND40 = [
    (dict(kmin=31, kmax=31), [3, 9, 22, 28, 35, 26, 12, 25, 5, 37, 15, 13], [(3, 1350, 1350), (9, 814, 1876)], (39, 0, 2100)),      # `memo panel -k 31`
    (dict(), [26, 9, 39, 29, 13, 35, 30, 25, 33, 27, 14, 20],
     [(26, 82586, 82586), (9, 58431, 106159), (39, 44549, 118861), (29, 38917, 126593), (13, 35329, 132810)], (11, 11852, 164613)),
    (dict(objective="core"), [26, 13, 9, 3, 32, 34, 19, 35, 24, 28, 11, 33], [(26, 82586, 82586), (13, 59227, 101339), (9, 48808, 117007)], (27, 11852, 164613)),
    (dict(kmax=64), _K64, [(9, 79659, 79659), (3, 58505, 99889), (26, 47664, 110213), (7, 40841, 115889), (27, 35107, 120260)], (28, 11852, 133819)),
    (dict(kmin=12, kmax=64), _K64, [(9, 57070, 57070), (3, 36111, 76814)], (28, 223, 110719)),
    (dict(kmax=64, objective="core"), [9, 3, 25, 13, 26, 32, 19, 34, 2, 33, 7, 11], [(9, 79659, 79659), (3, 58505, 99889), (25, 47992, 108729)], (27, 11852, 133819)),
]

# stopping on rnd_n40.parquet at -K 64, where L x span is 134400: (flags, genome lines)
RND40_STOPS = [
    (dict(kmax=64, fraction="0.9"), 6),
    (dict(kmax=64, fraction="0.5"), 1),
]

# `memo cover -b example_memb.parquet -n 5 -r ref_1:0-20 -K 8`: the README's bytes
README_EXAMPLE = "genomes\tcore\tcovered\tadded\n1\t160\t0\t0\n2\t83\t83\t3\n3\t72\t93\t2\n4\t59\t94\t4\n5\t49\t95\t1\n"
