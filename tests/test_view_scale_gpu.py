"""`memo view` at the sizes it was written for: the device reader of conservation text (memo_text.hip) past one wave and one trip
of its scan, at whole tiles and across tile edges, and the histogram (bin_conservation_kernel, memo_index.hip) with more than one
slice per bin, bin by bin.  test_view_gpu.py holds the grammar; this module holds the structure.  What each group is there for:

  A  text_scan_kernel: the cross-wave term (`before`, wsum[]) from the 65th tile on, and `carry` between trips of 1024 tiles --
     added to a non-zero carry from the 2049th tile on.  Prefixes of 64 / 65 / 1024 / 1025 tiles end on each side of both edges.
  B  the launcher's nbytes / 16384 + 1 tiles: the last tile that is empty (a text of whole tiles that \\n ends) or holds nothing
     but the staged terminator (one that no \\n ends), at the first tile of a wave and of a trip; load_chunk's tail on texts
     shorter than the halo, than one 16-byte load, and at 15, 16 and 17 bytes.  (The + 1 as such is no gap: without it any text
     that is not whole tiles loses its partial last tile, and test_view_gpu.py notices.  What they never launch is the tile
     behind a text of whole tiles.)
  C  text_parse_kernel's 48-byte halo and text_count_kernel's look across the tile's edge (j == 15): every line form with its
     terminator at every offset from -35 to +35 around a tile boundary, \\r on a tile's last byte and the whole 34 bytes of halo
     included, at boundaries in every wave of the scan.
  D  first_odd_offset (both kernels' atomicMin): every oddity with each of its bytes on a tile's last byte, far into the text; the
     smaller of two offsets found by different workgroups, waves and kernels; and a seeded differential against the contract of
     include/memo_amd_dap.h, written down here line by line.
  E  bin_conservation_kernel, every count in its own bin: the LDS histogram with 8, 174 and 244 slices a bin, the global-atomic
     path, the last LDS and the first global num_docs (12287 / 12288), slices that begin past their bin's end, an empty bin, edges
     that do not span the vector, and memo_bin_conservation_dev's refusals; then a vector that a sweep left in HBM.
     (Counts that a slice loses, as with a floored slice width, the column sums of test_gpu_parity.py already notice on the
     global path; counts in the wrong bin, and anything on the LDS path with more than one slice, only these do.)
  F  the whole text route at size: a file of more than 1025 tiles, memory-mapped, through memo_dev_upload_pipelined in many pieces,
     parsed and binned on the device (view.preprocess_data).

Every expected value is the reference's own reading of the same bytes (reference_reading, plot_conservation.py:40-49), numpy
written here, or oracle.view_table: none comes from the library."""
import ctypes as C

import numpy as np
import pytest

from tests.test_view_gpu import ODDITIES, parse_on_device, reference_reading

pytestmark = pytest.mark.gpu

TILE = 16384


@pytest.fixture(scope="module")
def memo():
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()                     # make: a no-op when libmemo_amd.so is up to date
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return memo_amd


def tiles_of(nbytes):
    return nbytes // TILE + 1            # the launcher's grid (memo_text.hip)


# ---- in-grammar text, to the byte ------------------------------------------------------------------------------------------------
BLANKS = (b" ", b"\t")


def content(length, rng):
    """one line of the grammar without its terminator, exactly `length` bytes (1 - 32): [ \\t]*[0-9]{1,9}[ \\t]*"""
    assert 1 <= length <= 32
    nd = int(rng.integers(1, min(length, 9) + 1))
    left = int(rng.integers(0, length - nd + 1))
    pad = [BLANKS[i] for i in rng.integers(0, 2, length - nd)]
    return b"".join(pad[:left]) + "".join(map(str, rng.integers(0, 10, nd))).encode() + b"".join(pad[left:])


def compose(n, closed, rng, longest=12):
    """exactly n bytes of in-grammar lines of at most `longest` bytes (+ \\n or \\r\\n); closed: the last one ends in \\n"""
    assert n >= (2 if closed else 1)
    out, r = [], n
    while r:
        if not closed and r <= longest and (r < 3 or rng.random() < 0.5):
            out.append(content(r, rng))                                  # the open last line
            break
        k = int(rng.integers(2, min(r if closed else r - 1, longest + 1) + 1))      # a line with its terminator
        if closed and r - k == 1:
            k += 1                                                       # (one byte left over could hold no line)
        out.append(content(k - 2, rng) + b"\r\n" if k >= 3 and rng.random() < 0.25 else content(k - 1, rng) + b"\n")
        r -= k
    data = b"".join(out)
    assert len(data) == n
    return data


def whole_lines(data, nbytes):
    """(exactly nbytes >= 2 of whole in-grammar lines, how many of them are data's own bytes): a prefix of the in-grammar `data`
    cut at a line's end, then lines of blanks and a 5"""
    keep = data.rfind(b"\n", 0, nbytes - 2) + 1                          # 0 where no line of data's ends that early
    gap, out = nbytes - keep, [data[:keep]]
    while gap > 33:
        out.append(b" " * 14 + b"5\n")
        gap -= 16
    out.append(b" " * (gap - 2) + b"5\n")                                # 2 <= gap <= 33: a line of 32 bytes at most
    text = b"".join(out)
    assert len(text) == nbytes
    return text, keep


class Filler:
    """in-grammar filler of any exact length: a pool composed once (Python composes 10^5 lines a second), repeated and cut by
    whole_lines; an open one is a closed one of one byte more without its last \\n"""

    def __init__(self, seed, longest=12):
        self.pool = compose(2 * TILE + 1001, True, np.random.default_rng(seed), longest)

    def __call__(self, n, closed=True):
        if n == 0 and closed:
            return b""
        if not closed:
            return self(n + 1)[:-1]
        return whole_lines(self.pool * (n // len(self.pool) + 1), n)[0]


def read_as_the_reference(data, tmp_path):
    path = tmp_path / "c.txt"
    path.write_bytes(data)
    return reference_reading(str(path))


def assert_reading(data, want, where=""):
    """the device's reading of these bytes is `want`; on a mismatch: the first differing line and the tile that holds it"""
    vec, lines, odd = parse_on_device(data)
    assert (lines, odd) == (len(want), -1), (where, len(data), tiles_of(len(data)))
    if not np.array_equal(vec, want):
        i = int(np.flatnonzero(vec != want)[0])
        ends = np.flatnonzero(np.frombuffer(data, np.uint8) == 10)
        at = int(ends[i]) if i < len(ends) else len(data)                # the line's terminator: its tile numbers it
        pytest.fail(f"{where}: line {i} of {len(want)} reads {vec[i]}, not {want[i]}; its terminator is byte {at}, "
                    f"tile {at // TILE} (wave {at // TILE % 1024 // 64} of trip {at // TILE // 1024} of the scan), "
                    f"byte {at % TILE} of it; {int((vec != want).sum())} lines differ")


# ---- A. line numbering past one wave and past one scan trip --------------------------------------------------------------------------
BIG_TILES = 2112                         # the scan's third trip adds to a carry that is not zero


@pytest.fixture(scope="module")
def big_text(tmp_path_factory):
    """(bytes, the reference's reading of them): 2112 tiles of mixed forms -- plain, zero-padded, blank- and tab-padded, one
    line in eight CRLF -- padded to some 16 bytes a line, so 2 * 10^6 lines"""
    rng = np.random.default_rng(2024)
    n = 2_300_000
    values = rng.integers(0, 70000, n)                                   # 1 - 5 digits; one in fifteen is 65535 or more
    pads = [b"", b" ", b"\t ", b" \t ", b"\t\t   ", b"        ", b" \t \t \t \t  ", b"\t           ", b"            ", b"\t\t\t\t\t\t\t\t\t\t\t\t"]
    assert max(map(len, pads)) == 12 and max(map(len, pads[:7])) == 10   # 12 + (4 + 5 digits) + 10 = 31 bytes at most
    left = rng.integers(0, len(pads), n).tolist()
    right = rng.integers(0, 7, n).tolist()
    zeros = rng.integers(0, 5, n).tolist()
    ends = [b"\r\n" if c else b"\n" for c in (rng.integers(0, 8, n) == 0).tolist()]
    form = rng.integers(0, 8, n).tolist()                                # one in eight plain, one in eight zero-padded only
    digits = [b"%d" % v for v in values.tolist()]
    data = b"".join([digits[i] + ends[i] if form[i] == 0 else
                     b"0" * zeros[i] + digits[i] + ends[i] if form[i] == 1 else
                     pads[left[i]] + b"0" * zeros[i] + digits[i] + pads[right[i]] + ends[i] for i in range(n)])
    assert len(data) > BIG_TILES * TILE
    cut = data.rindex(b"\n", 0, BIG_TILES * TILE - 100) + 1              # whole lines, \n the last byte
    data = data[:cut]
    assert tiles_of(len(data)) == BIG_TILES > 2048
    path = tmp_path_factory.mktemp("big") / "big.txt"
    path.write_bytes(data)
    want = reference_reading(str(path))
    assert 1_500_000 < len(want) < 3_000_000 and (want == 65535).sum() > 50_000 and want.max() == 65535
    want.setflags(write=False)
    return data, want


def test_reader_numbers_lines_past_two_scan_trips(memo, big_text):
    data, want = big_text
    assert_reading(data, want, "2112 tiles")


@pytest.mark.parametrize("ntiles", [64, 65, 1024, 1025])
def test_reader_prefix_of(memo, big_text, ntiles, tmp_path):
    """the same bytes cut just behind a digit, so still in grammar and open-ended: the last tile (the first of a wave, of a
    trip, or the last of either) holds a few bytes and the staged terminator"""
    data, want = big_text
    cut = (ntiles - 1) * TILE + 5
    while not 48 <= data[cut - 1] < 58:
        cut += 1
    assert tiles_of(cut) == ntiles and cut % TILE < 48
    whole = data.count(b"\n", 0, cut)
    last = read_as_the_reference(data[data.rindex(b"\n", 0, cut) + 1:cut], tmp_path)     # the line that was cut short
    assert len(last) == 1
    assert_reading(data[:cut], np.concatenate([want[:whole], last]), f"prefix of {ntiles} tiles")


# ---- B. texts that are whole tiles, and the shortest texts -------------------------------------------------------------------------
@pytest.mark.parametrize("closed", [True, False], ids=["closed", "open"])
@pytest.mark.parametrize("m", [1, 64, 1024])
def test_reader_text_of_whole_tiles(memo, big_text, m, closed, tmp_path):
    """nbytes == m * 16384: tile m is empty (closed) or holds only the staged terminator (open), and at m = 64 it is the first
    of a wave, at m = 1024 the first of a trip: its base is the carry alone"""
    data, want = big_text
    text, keep = whole_lines(data, m * TILE - 27)
    text += b"\t" * 20 + (b"654321\n" if closed else b"7654321")
    assert len(text) == m * TILE and tiles_of(len(text)) == m + 1 and text.endswith(b"\n") == closed
    whole = data.count(b"\n", 0, keep)
    assert_reading(text, np.concatenate([want[:whole], read_as_the_reference(text[keep:], tmp_path)]), f"{m} whole tiles")


def test_reader_every_length_from_1_to_70(memo, tmp_path):
    """below the 48-byte halo, below one 16-byte load, at 15, 16 and 17; a closed text has two bytes at least (a lone \\n is a
    blank line: odd at byte 0, and the reference refuses it too)"""
    rng = np.random.default_rng(31)
    for n in range(1, 71):
        for closed in (True, False):
            if closed and n == 1:
                assert parse_on_device(b"\n")[1:] == (1, 0)
                with pytest.raises(ValueError):
                    read_as_the_reference(b"\n", tmp_path)
                continue
            for longest in (5, 30):
                data = compose(n, closed, rng, longest)
                assert_reading(data, read_as_the_reference(data, tmp_path), f"{n} bytes: {data!r}")


# ---- C. every line form at every offset across a tile boundary ----------------------------------------------------------------------
FORMS = {"plain": b"123\n", "crlf": b"123\r\n", "blanks_both_sides": b" \t 123\t \t\n", "one_byte": b"7\n",
         "longest": b" " * 20 + b"123456789" + b"\t" * 3 + b"\n",         # 32 bytes and nine digits
         "longest_crlf": b"\t" * 11 + b"987654321" + b" " * 12 + b"\r\n"}  # ... and \r: all 34 bytes of halo are needed
OFFSETS = range(-35, 36)                 # of the terminator from the boundary: 0 is the next tile's first byte, -1 this one's last


def test_reader_every_form_at_every_offset_across_a_tile_boundary(memo, tmp_path):
    """one text, a different (form, offset) at each of its 426 tile boundaries, shuffled so that every form meets every wave of
    the scan; short in-grammar lines in between"""
    assert len(FORMS["longest"]) == 33 and len(FORMS["longest_crlf"]) == 34
    fill = Filler(41, longest=9)
    probes = [(f, d) for f in FORMS for d in OFFSETS]
    order = np.random.default_rng(42).permutation(len(probes))
    parts, size, placed = [], 0, []
    for boundary, i in enumerate(order, 1):
        form, d = probes[i]
        line = FORMS[form]
        start = boundary * TILE + d + 1 - len(line)                       # the line's first byte
        parts += [fill(start - size), line]
        size = start + len(line)
        placed.append((size - 1, form, d))
    parts.append(fill(3000))
    data = b"".join(parts)
    assert tiles_of(len(data)) == len(probes) + 1 >= 66
    for end, form, d in placed:
        assert data[end] == 10 and end == (end + 35) // TILE * TILE + d and data[end - len(FORMS[form])] == 10
    assert {f for e, f, d in placed if e // TILE >= 64} == set(FORMS)    # past wave 0 of the scan: every form
    at = {e: (f, d) for e, f, d in placed}
    e = next(e for e in at if at[e] == ("crlf", 0))
    assert e % TILE == 0 and data[e - 1] == 13                           # \r on a tile's last byte, its \n in the next
    e = next(e for e in at if at[e] == ("longest_crlf", 0))
    assert e % TILE == 0 and data[e - 34] == 10                          # ... and behind it 34 bytes of halo, all needed
    want = read_as_the_reference(data, tmp_path)
    vec, lines, odd = parse_on_device(data)
    assert (lines, odd) == (len(want), -1)
    if not np.array_equal(vec, want):
        ends = np.flatnonzero(np.frombuffer(data, np.uint8) == 10)
        wrong = [(at[int(ends[i])], int(vec[i]), int(want[i])) for i in np.flatnonzero(vec != want) if int(ends[i]) in at]
        i = int(np.flatnonzero(vec != want)[0])
        pytest.fail(f"{int((vec != want).sum())} lines differ, the first is line {i} in tile {int(ends[i]) // TILE}; "
                    f"probes among them ((form, offset), got, want): {wrong[:20]}")


# ---- D. oddities across a tile boundary and far into a text ------------------------------------------------------------------------
def first_odd_offset_reference(data):
    """The contract of include/memo_amd_dap.h, as it is written there.  A byte offends at its own offset when it is no digit,
    blank, \\t, \\r or \\n, or is a \\r that no \\n follows directly.  A line -- what \\n, \\r\\n or the end of the text ends --
    offends at the offset of its terminator (nbytes for a last line without \\n) when it is empty or blanks only, has blanks
    between digits, ten or more digits, or more than 32 bytes.  The smallest offset, -1 when nothing offends."""
    n = len(data)
    a = np.frombuffer(data, np.uint8)
    in_grammar = np.zeros(256, bool)
    in_grammar[list(b"0123456789 \t\r\n")] = True
    bad = ~in_grammar[a] | ((a == 13) & (np.append(a[1:], 0) != 10))
    first = int(np.flatnonzero(bad)[0]) if bad.any() else -1
    start = 0
    while start < n and (first < 0 or start < first):                    # (a later line can only offend later)
        end = data.find(b"\n", start)
        end = n if end < 0 else end
        line = data[start:end]
        if end < n and line.endswith(b"\r"):
            line = line[:-1]                                             # \r\n ends it
        bare = line.strip(b" \t")
        digits = sum(48 <= c < 58 for c in bare)
        if len(line) > 32 or not bare or b" " in bare or b"\t" in bare or digits >= 10:
            return end if first < 0 or end < first else first
        start = end + 1
    return first


def test_the_reference_of_the_contract_on_the_oddities_of_the_grammar_tests():
    """no device here: the differential's reference on cases whose answer is known by hand (under the module's gpu mark with the
    tests that lean on it, so it runs where they run)"""
    for name, oddity, at in ODDITIES:
        for tail in (b"8\n9\n", b""):
            assert first_odd_offset_reference(b"12\n345\r\n" + oddity + tail) == 8 + at, name
    for data, want in ((b"", -1), (b"7", -1), (b"7\n", -1), (b" 7\t\r\n8", -1), (b"7\r", 1), (b"1 2", 3), (b"\n", 0), (b"5\n ", 3),
                       (b"5\n\n+", 2), (b"+\n\n", 0), (b" " * 23 + b"123456789", -1), (b" " * 24 + b"123456789", 33),
                       (b" " * 23 + b"123456789\r\n", -1), (b"1\r\r\n", 1), (b"0000000001\n", 10), (b"\xff", 0)):
        assert first_odd_offset_reference(data) == want, data


@pytest.fixture(scope="module")
def head65(big_text):
    """in-grammar lines up to the end of tile 64 and a little more"""
    return big_text[0][:65 * TILE + 100]


@pytest.mark.parametrize("name,oddity,at", ODDITIES, ids=[o[0] for o in ODDITIES])
def test_reader_reports_an_oddity_across_a_tile_boundary(memo, head65, name, oddity, at):
    """each byte of the oddity in turn is the last byte of tile 64, the first tile of the scan's second wave"""
    edge = 65 * TILE - 1
    for i in range(len(oddity)):
        head = whole_lines(head65, edge - i)[0]
        for tail in (b"8\n9\n", b""):
            data = head + oddity + tail
            assert data[edge] == oddity[i] and (len(head) + at) // TILE in (64, 65)
            assert parse_on_device(data)[2] == len(head) + at, (name, i, tail)


def test_reader_cr_on_a_tiles_last_byte_and_no_newline_behind_it(memo, head65):
    edge = 65 * TILE - 1
    head = whole_lines(head65, edge - 1)[0]
    for follower in (b"6\n", b" \n", b"\r\n", b"\t7\n", b"\x00\n"):
        data = head + b"5\r" + follower + b"8\n"
        assert data[edge] == 13 and data[edge + 1] != 10
        assert parse_on_device(data)[2] == edge, follower
    data = head + b"5\r\n8\n"                                            # ... and with it: nothing odd
    assert parse_on_device(data)[1:] == (data.count(b"\n"), -1)


def test_reader_line_of_33_bytes_ending_on_a_tiles_first_byte(memo, head65):
    edge = 65 * TILE
    head = whole_lines(head65, edge - 33)[0]
    for line in (b" " * 24 + b"123456789", b"12345" + b"\t" * 28, b" " * 33, b" " * 31 + b"7\r"):
        data = head + line + b"\n8\n"
        assert data[edge] == 10 and len(line) == 33
        want = -1 if line.endswith(b"\r") else edge                      # 32 bytes and \r\n: inside the grammar
        assert parse_on_device(data)[2] == want, line


def test_reader_of_two_oddities_reports_the_smaller_offset(memo, big_text):
    """in different tiles and waves of one text, and in tiles 1 and 1500 of one; a byte that text_count_kernel finds against a
    line that text_parse_kernel finds, either first"""
    data, _ = big_text
    byte_odd, line_odd = b"4_2\n", b"1 2\n"                               # odd at +1 (the byte), at +3 (the line's terminator)
    for (tile_a, in_a), (tile_b, in_b), size in (((3, 100), (70, 2 * 4096 + 100), 72), ((70, 3 * 4096 + 900), (3, 4096 + 500), 72),
                                                 ((1, 5000), (1500, 9000), 1502), ((1500, 120), (1, 16000), 1502)):
        for first, second in ((byte_odd, line_odd), (line_odd, byte_odd)):
            text = bytearray(data[:data.rindex(b"\n", 0, size * TILE - 1) + 1])
            where = []
            for oddity, tile, within in ((first, tile_a, in_a), (second, tile_b, in_b)):
                start = data.rindex(b"\n", 0, tile * TILE + within) + 1   # written over whole lines: the oddity, then blanks and a 3
                end = data.index(b"\n", start) + 1
                while end - start < len(oddity) + 2:
                    end = data.index(b"\n", end) + 1
                text[start:end] = oddity + b" " * (end - start - len(oddity) - 2) + b"3\n"
                assert start // TILE == end // TILE == tile and end - start - len(oddity) <= 33
                where.append(start + (1 if oddity is byte_odd else 3))
            assert tiles_of(len(text)) == size and where[0] // TILE == tile_a and where[1] // TILE == tile_b
            if size < 100:
                assert first_odd_offset_reference(bytes(text)) == min(where)
            assert parse_on_device(bytes(text))[2] == min(where), (tile_a, tile_b, first)


INJECTED = [b"\n", b" \t \n", b"  \r\n", b"1 2\n", b"12\t3 \n", b"1234567890\n", b"00000000012\n", b" " * 30 + b"123\n",
            b"7" + b"\t" * 32 + b"\n", b" " * 32 + b"\n", b"+1\n", b"-5\n", b"1_0\n", b"5\r6\n", b"4\x00\n", b"\xc3\xa9\n", b"0x1F\n"]


def random_text(rng, fill):
    """(1 - 5 tiles of in-grammar lines, closed or open, with zero to three things injected; what was injected where): lines of
    INJECTED between two lines, and bytes (any byte; a lone \\r) written over whatever lies there -- each at random or with one
    of its bytes on, before or behind a tile boundary"""
    size = int(rng.integers(2, 5 * TILE))
    edges = list(range(TILE, size, TILE))

    def place(length):
        if edges and rng.random() < 0.6:
            return max(0, int(rng.choice(edges)) - int(rng.integers(0, length + 2)))
        return int(rng.integers(0, max(size - length, 1)))
    as_line = rng.random(int(rng.integers(0, 4))) < 0.6
    lines = sorted((place(len(o)), o) for o in (INJECTED[int(rng.integers(0, len(INJECTED)))] for _ in range(int(as_line.sum()))))
    parts, at, what = [], 0, []
    for start, oddity in lines:
        if start < at or start - at == 1:                                # (no room for a line before it)
            continue
        parts += [fill(start - at), oddity]
        at = start + len(oddity)
        what.append((start, oddity))
    if size - at >= 2:
        parts.append(fill(size - at, closed=bool(rng.integers(0, 2))))
    text = bytearray(b"".join(parts))
    for _ in range(int((~as_line).sum())):
        p = min(place(1), len(text) - 1)
        text[p] = 13 if rng.random() < 0.4 else int(rng.integers(0, 256))
        what.append((p, bytes(text[p:p + 1])))
    return bytes(text), what


@pytest.mark.parametrize("seed", [50, 51, 52, 53])
def test_reader_differential_against_the_contract(memo, seed, tmp_path):
    rng = np.random.default_rng(seed)
    fill = Filler(seed + 100, longest=20)
    clean = 0
    for case in range(75):
        data, what = random_text(rng, fill)
        want = first_odd_offset_reference(data)
        vec, lines, odd = parse_on_device(data)
        assert odd == want, f"seed {seed} case {case}: {len(data)} bytes, injected (offset, bytes) {what}: " \
                            f"{data[max(want, odd, 40) - 40:max(want, odd) + 8]!r}"
        if odd == -1:
            clean += 1
            reading = read_as_the_reference(data, tmp_path)
            assert lines == len(reading) and np.array_equal(vec, reading), f"seed {seed} case {case}: {what}"
    assert 5 <= clean <= 60                                              # both kinds in numbers


def test_reader_refuses_text_that_is_not_16_byte_aligned(memo):
    from memo_amd._lib import MEMO_EINVAL, check, lib
    d_text, d_vec = C.c_void_p(), C.c_void_p()
    check(lib().memo_dev_malloc(0, 4096, C.byref(d_text)))
    check(lib().memo_dev_malloc(0, 4096, C.byref(d_vec)))
    try:
        assert d_text.value % 16 == 0
        for shift in (1, 8, 15):
            lines, odd = C.c_int64(-7), C.c_int64(-7)
            rc = lib().memo_parse_conservation_text_dev(C.c_void_p(d_text.value + shift), 100, d_vec, 2048, C.byref(lines),
                                                        C.byref(odd), 0, None)
            assert (rc, lines.value, odd.value) == (MEMO_EINVAL, 0, -1), shift
    finally:
        lib().memo_dev_free(0, d_text)
        lib().memo_dev_free(0, d_vec)


# ---- E. binning: per-bin counts on both paths, more than one slice -----------------------------------------------------------------
def counts_reference(vec, edges, n_docs):
    """[n_bins, n_docs + 1]: position p lies in the bin whose edges enclose it; a value above n_docs is counted in no column"""
    vec, edges = np.asarray(vec, np.int64), np.asarray(edges, np.int64)
    n_bins, ncols = len(edges) - 1, n_docs + 1
    bins = np.searchsorted(edges, np.arange(len(vec)), "right") - 1
    keep = (bins >= 0) & (bins < n_bins) & (vec <= n_docs)
    return np.bincount(bins[keep] * ncols + vec[keep], minlength=n_bins * ncols).reshape(n_bins, ncols).astype(np.uint64)


def reference_edges(L, n_bins):
    return np.array([int(x) for x in np.linspace(0, L, n_bins + 1)], np.int64)     # plot_conservation.py:52


def slices_of(L, n_bins):
    """memo_bin_conservation_dev's rule: enough workgroups to fill the chip, 4096 positions each at least"""
    slices, longest = (2048 + n_bins - 1) // n_bins, (L + n_bins - 1) // n_bins
    while slices > 1 and longest // slices < 4096:
        slices -= 1
    return slices


def seeded_vector(L, n_docs, seed):
    """every value of 0 .. n_docs, and one position in sixteen out of range: n_docs + 1, 40000 and 65535 among them"""
    rng = np.random.default_rng(seed)
    vec = rng.integers(0, n_docs + 1, L).astype(np.uint16)
    out = rng.random(L) < 1 / 16
    vec[out] = rng.choice(np.array([n_docs + 1, 40000, 65535, 65534], np.uint16), int(out.sum()))
    return vec


def assert_bin_counts(view, vec, n_docs, n_bins, slices):
    L = len(vec)
    assert slices_of(L, n_bins) == slices > 1
    counts, edges = view.bin_counts(vec, n_docs, n_bins)
    want_edges = reference_edges(L, n_bins)
    want = counts_reference(vec, want_edges, n_docs)
    assert np.array_equal(edges, want_edges) and counts.dtype == np.uint64 and counts.shape == want.shape
    in_range = np.add.reduceat((vec <= n_docs).astype(np.int64), want_edges[:-1])
    assert np.array_equal(want.sum(1), in_range) and in_range.sum() < L  # (a row is the bin's values in range, not its width)
    if not np.array_equal(counts, want):
        b, v = (int(x[0]) for x in np.nonzero(counts != want))
        pytest.fail(f"n_docs {n_docs}, {n_bins} bins of {L}, {slices} slices: {int((counts != want).sum())} counts differ, the "
                    f"first in bin {b}, value {v}: {counts[b, v]}, not {want[b, v]}; row sums {counts.sum(1)[:8]} for {in_range[:8]}")


# the slice counts are the launcher's rule worked out by hand: 2048 / bins workgroups a bin, fewer until each has 4096 positions
@pytest.mark.parametrize("n_docs,n_bins,L,slices", [(100, 3, 100_003, 8),         # 33335 / 8 = 4166; ragged: 33334 = 8 * 4167 - 2
                                                    (100, 1, 1_000_003, 244),     # 1000003 / 244 = 4098
                                                    (100, 7, 5_000_000, 174)],    # 714286 / 174 = 4105
                         ids=["3_bins_8_slices", "1_bin_244_slices", "7_bins_174_slices"])
def test_bin_counts_lds_path_many_slices(memo, n_docs, n_bins, L, slices):
    from memo_amd import view
    assert (n_docs + 1) * 4 <= 48 * 1024
    assert_bin_counts(view, seeded_vector(L, n_docs, 60 + n_bins), n_docs, n_bins, slices)


def test_bin_counts_global_path_per_bin(memo):
    from memo_amd import view
    assert (20000 + 1) * 4 > 48 * 1024
    assert_bin_counts(view, seeded_vector(100_000, 20000, 64), 20000, 3, 8)      # 33334 / 8 = 4166


def test_bin_counts_at_the_48_kb_boundary_between_the_paths(memo):
    """num_docs 12287 is the last whose columns fit the LDS histogram ((12287 + 1) * 4 == 48 KB), 12288 the first on global atomics"""
    from memo_amd import view
    assert (12287 + 1) * 4 == 48 * 1024
    vec = seeded_vector(100_003, 12289, 65)                              # 12288 and 12289 among the values
    assert (vec == 12288).any() and (vec == 12289).any()
    for n_docs in (12287, 12288):
        assert_bin_counts(view, vec, n_docs, 3, 8)


def bin_directly(vec, L, edges, n_docs, n_bins=None):
    """(return code, counts) of memo_bin_conservation_dev; counts is 0xA5 in every byte beforehand"""
    from memo_amd._lib import check, lib
    edges = np.asarray(edges, np.int64)
    n_bins = len(edges) - 1 if n_bins is None else n_bins
    counts = np.full((max(n_bins, 1), n_docs + 1 if n_docs < 65535 else 1), 0xA5A5A5A5A5A5A5A5, np.uint64)
    d_vec = C.c_void_p()
    if len(vec):
        host = np.ascontiguousarray(vec, np.uint16)
        check(lib().memo_dev_malloc(0, host.nbytes, C.byref(d_vec)))
        check(lib().memo_dev_upload(0, d_vec, host.ctypes.data, host.nbytes, None))
    try:
        rc = lib().memo_bin_conservation_dev(d_vec, L, edges.ctypes.data, n_bins, n_docs, counts.ctypes.data, 0, None)
    finally:
        if len(vec):
            lib().memo_dev_free(0, d_vec)
    return rc, counts


def test_bin_conservation_dev_with_hand_made_edges(memo):
    from memo_amd._lib import MEMO_EINVAL, MEMO_OK
    n_docs, L = 100, 100_003
    vec = seeded_vector(L, n_docs, 66)
    a = 41_234
    for edges, slices in (([0, 5, L], 12),             # a bin of 5 in 12 slices of one position: seven begin past its end
                          ([0, a, a, L], 8),           # an empty bin between full ones
                          ([17, L - 9], 24),           # edges that do not span the vector
                          ([0, 1, 2, 4099, 4100, L - 1, L - 1, L], 3)):
        assert slices_of(L, len(edges) - 1) == slices > 1
        rc, counts = bin_directly(vec, L, edges, n_docs)
        want = counts_reference(vec, edges, n_docs)
        assert rc == MEMO_OK and want.sum() > 0.9 * (edges[-1] - edges[0])
        assert np.array_equal(counts, want), (edges, np.argwhere(counts != want)[:5].tolist())
    for n in (n_docs, 20000):                            # both paths
        rc, counts = bin_directly(vec[:0], 0, [0, 0], n)
        assert rc == MEMO_OK and counts.shape == (1, n + 1) and not counts.any()
        rc, counts = bin_directly(vec, L, [0, 5, L], n)
        assert rc == MEMO_OK and np.array_equal(counts, counts_reference(vec, [0, 5, L], n))
    untouched = np.uint64(0xA5A5A5A5A5A5A5A5)
    for edges, n, n_bins, why in (([0, 50_000, 40_000, L], n_docs, None, "decreasing edges"),
                                  ([0, 50_000, L + 1], n_docs, None, "an edge past L"),
                                  ([-1, 50_000, L], n_docs, None, "an edge before 0"),
                                  ([0, L], n_docs, 0, "no bins"),
                                  ([0, L], 0, None, "no genomes"),
                                  ([0, L], 65535, None, "65535 is the value that stands for out of range")):
        rc, counts = bin_directly(vec, L, edges, n, n_bins)
        assert rc == MEMO_EINVAL and (counts == untouched).all(), why


def test_bin_counts_of_a_vector_the_sweep_left_in_hbm(memo, oracle):
    """the device-pointer form, as view.preprocess_region uses it: conservation_dev into a uint16 buffer, binned where it lies"""
    from memo_amd import synth, view
    from memo_amd._lib import check, lib
    n, L, k = 100, 300_000, 31
    ix, _ = synth.device_index(0, L, k, n, L)
    d_vec = C.c_void_p()
    check(lib().memo_dev_malloc(0, 2 * L, C.byref(d_vec)))
    try:
        with ix:
            ix.conservation_dev(0, L, k, n, d_vec.value)
            ix.check()
            vec = ix.conservation(0, L, k, n)                            # the same sweep, downloaded
            assert vec.dtype == np.uint16 and len(np.unique(vec)) > 10
            for n_bins in (1, 4, 500):
                counts, edges = view.bin_counts((d_vec.value, L), n, n_bins)
                assert np.array_equal(edges, reference_edges(L, n_bins))
                assert np.array_equal(counts, counts_reference(vec, edges, n)), n_bins
                got, want = view._table(counts, edges, n, n_bins), oracle.view_table(vec, n, n_bins)
                for key in want:
                    assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), (n_bins, key)
    finally:
        lib().memo_dev_free(0, d_vec)


# ---- F. end to end at size ----------------------------------------------------------------------------------------------------------
def test_text_route_end_to_end_past_1025_tiles(memo, oracle, tmp_path):
    """emit_conservation's text of 4.2 * 10^6 values: memory-mapped, uploaded in pieces, parsed and binned on the device"""
    from memo_amd import view
    n_docs, L = 30, 4_200_000
    rng = np.random.default_rng(70)
    vec = rng.integers(0, n_docs + 1, L).astype(np.uint16)
    far = rng.random(L) < 0.5
    vec[far] = rng.integers(40000, 65536, int(far.sum())).astype(np.uint16)        # five digits; in no column of the table
    vec[:3] = (n_docs + 1, 65535, 65534)
    path = tmp_path / "out.txt"
    path.write_bytes(memo.emit_conservation(vec))
    assert tiles_of(path.stat().st_size) > 1025
    with open(path, "rb") as f:
        assert f.read(15) == b"31\n65535\n65534\n"
    for n_bins in (3, 500):
        got, want = view.preprocess_data(str(path), n_docs, n_bins), oracle.view_table(vec, n_docs, n_bins)
        for key in want:
            assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), (n_bins, key)
