"""The worked tables of `memo panel` (README), shared by tests/test_panel_cpu.py (the oracle against them) and
tests/test_panel_gpu.py (the device against them).  Rows are (added, core, covered).  They were computed on the CPU by a NumPy
greedy on memo_oracle.np_membership bits of the committed goldens."""

# example_memb.parquet, -n 5 -r ref_1:0-20: (k, flags of region_panel, rows)
EXAMPLE = [
    (3, dict(), [(3, 20, 20), (4, 18, 20), (2, 16, 20), (1, 8, 20)]),
    (3, dict(objective="core"), [(3, 20, 20), (4, 18, 20), (2, 16, 20), (1, 8, 20)]),
    (3, dict(candidates="1,2,4"), [(4, 18, 18), (1, 8, 20), (2, 8, 20)]),
    (3, dict(seeds="1"), [(1, 10, 10), (3, 10, 20), (2, 8, 20), (4, 8, 20)]),
    (3, dict(fraction="0.7"), [(3, 20, 20)]),
    (3, dict(max_genomes=2), [(3, 20, 20), (4, 18, 20)]),
    (4, dict(), [(2, 12, 12), (3, 10, 14), (4, 3, 15), (1, 1, 16)]),          # genomes 2 and 3 tie at new = kept = 12: the annot decides
    (4, dict(candidates="1,2,4"), [(2, 12, 12), (4, 5, 13), (1, 1, 14)]),
    (4, dict(seeds="1"), [(1, 2, 2), (2, 1, 13), (3, 1, 15), (4, 1, 16)]),
    (4, dict(fraction="0.7"), [(2, 12, 12), (3, 10, 14)]),
    (5, dict(), [(3, 8, 8), (2, 5, 10), (1, 0, 10), (4, 0, 10)]),
    (5, dict(fraction="0.7"), [(3, 8, 8), (2, 5, 10), (1, 0, 10), (4, 0, 10)]),  # the threshold of 14 is never reached
    (5, dict(seeds="1"), [(1, 0, 0), (3, 0, 8), (2, 0, 10), (4, 0, 10)]),
]

# rnd_n40.parquet, -n 40 -r chr1:0-2100: (k, flags, the order's first genomes, the first rows, the last row)
RND40 = [
    (31, dict(), [3, 9, 22, 28, 35, 26, 12, 25, 5, 37, 15, 13],
     [(3, 1350, 1350), (9, 814, 1876), (22, 378, 2052), (28, 214, 2092), (35, 148, 2100)], (39, 0, 2100)),
    (31, dict(objective="core"), [3, 4, 6, 27, 32, 38, 33, 2, 25, 14, 28, 1],
     [(3, 1350, 1350), (4, 819, 1726), (6, 501, 1854), (27, 314, 1996), (32, 195, 2033)], (37, 0, 2100)),
    (12, dict(), [3, 31, 34, 19, 7, 4, 21, 9, 5, 25, 36, 2], [(3, 2026, 2026), (31, 1871, 2100)], (22, 97, 2100)),
    (12, dict(objective="core"), [3, 34, 19, 4, 28, 24, 13, 33, 7, 9, 26, 21], [(3, 2026, 2026), (34, 1926, 2095), (19, 1822, 2100)], (27, 97, 2100)),
    (8, dict(), [34, 3, 19, 21, 26, 4, 28, 24, 33, 35, 5, 9], [(34, 2074, 2074), (3, 2045, 2100), (19, 2005, 2100)], (10, 504, 2100)),
    (8, dict(objective="core"), [34, 3, 19, 21, 26, 4, 28, 24, 33, 35, 5, 9], [(34, 2074, 2074), (3, 2045, 2100), (19, 2005, 2100)], (10, 504, 2100)),
]

# stopping on rnd_n40.parquet: (window, k, flags, lines, or the rows)
RND40_STOPS = [
    ((0, 2100), 31, dict(fraction="0.95"), 3),
    ((0, 2100), 31, dict(fraction="1"), 5),
    ((0, 2100), 8, dict(fraction="0.95"), 1),
    ((150, 450), 31, dict(fraction="1"), [(29, 237, 237), (22, 130, 299), (26, 103, 300)]),
]

# `memo panel -b example_memb.parquet -k 3 -n 5 -r ref_1:0-20`: the README's bytes
README_EXAMPLE = "genomes\tcore\tcovered\tadded\n1\t20\t0\t0\n2\t20\t20\t3\n3\t18\t20\t4\n4\t16\t20\t2\n5\t8\t20\t1\n"
