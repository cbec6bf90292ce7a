#!/usr/bin/env python3
"""`memo index`: FASTA genomes -> matching statistics on the GPU -> MEMO index rows -> Parquet, in one command.

    memo index -g genome_list.txt -o work -p test [-m]

Same command line, usage text and progress lines as the reference's src/index.sh, which builds the matching
statistics (MS) with MONI, genome by genome on the host.  Here every stage runs on the device:

  1. FASTA -> bytes (host, this module): a record's name is the first word after '>'; its sequence lines are
     joined with all whitespace removed and upper-cased.  The first genome of the list is the pivot; its record
     names and offsets take the place of the .fai that `samtools faidx` writes (index.sh:55-56).
  2. genome g's text (index.sh:63-65): S_1 $ S_2 $ ... S_s $ rc(S_1) $ ... rc(S_s) $, with $ a NUL byte (no
     pivot byte can be NUL: such input is refused) and rc the reverse complement of `samtools faidx -i`
     (A-T, C-G, R-Y, K-M, B-V, D-H swap, every other byte stays).  The records go to the device once, back to
     back; the device assembles the text in pieces, each a run of whole strings under the int32 suffix-array
     limit (the cap: MEMO_INDEX_PIECE_BYTES, else min(2^30, what the free device memory allows)).
  3. MS of every pivot position against every genome text (memo_ms_*, memo_amd/csrc/memo_ms.hip: suffix array,
     LCP, MS walk per piece), straight into the DAP matrix [positions][genomes - 1] in HBM (index.sh:83).  No
     match crosses a $, so the elementwise maximum over the pieces is the MS against the whole text, exactly.
     Where that matrix does not fit in the device's free memory (MEMO_INDEX_DAP_LAYOUT unset or `auto`; `dense` and
     `coded` force one), every column is kept run-coded instead -- MS falls by at most one per position, so a flag
     bit per position and the values of the flagged positions give it back exactly -- and stage 4 reads rows decoded
     on the device a batch at a time.  The index is the same file either way.
  4. DAP -> index rows on the device (memo_dap_push_dev; --mem --overlap, plus --order for the conservation
     index: index.sh:86-103) -> DIR/PREFIX.parquet (f0 utf8, f1 f2 f3 int64, ZSTD: parquet_compress_bed.py).

Not written, by design: MONI's *.w_rc* files, dap.txt, PREFIX.bed and the pivot's .fai.  Nothing downstream
reads them.

Refused with a message (never a wrong result): gzip input, a NUL byte, a pivot record of length 0, a pivot
record of 2^30 positions or more, a genome record of 2^31 - 2 bases or more (or longer than the piece cap less
one byte), more than 4096 genomes besides the pivot, a DAP that does not fit in the device's free memory even as
coded columns, a piece's working set that does not, a MEMO_INDEX_PIECE_BYTES that is not an integer in
[2, 2^31 - 2], a MEMO_INDEX_DAP_LAYOUT that is not auto, dense or coded, a MEMO_INDEX_WALK_BUDGET that is not an
integer >= 0 (the characters a match is extended one at a time before the rest is looked up by seed search; unset: the
library's default; 2^30 or more: never.  The index is the same file for every value).  A genome's whole
text may exceed 2^31 bytes: a human assembly (~6.2 GB of text) runs in a handful of pieces.
"""
import ctypes as C
import getopt
import os
import re
import sys
import time

import numpy as np

from ._lib import MemoError, check, lib

USAGE = """
omem index - index overlap order MEMs from a document array profile
Usage: omem index [options]

Basic options:
  -g [FILE]              document list
  -o [FILE]              output directory ['.']
  -p [FILE]              output file prefix
  -m                     make membership index

"""

SEPARATOR = b"\0"
_WHITESPACE = b" \t\r\n\v\f"
# samtools faidx -i: the IUPAC complement; every other byte (N, S, W, ...) is its own complement
_COMPLEMENT = bytes.maketrans(b"ACGTRYKMBVDH", b"TGCAYRMKVBHD")
MAX_RECORD = (1 << 30) - 1        # memo_dap: positions of one pivot record
MAX_TEXT = (1 << 31) - 2          # memo_ms: int32 suffix array of one genome text (and of one piece)
PIECE_ENV = "MEMO_INDEX_PIECE_BYTES"   # `memo index`: the piece cap (unset: the library's default)
MAX_COLUMNS = 4096                # memo_dap: genomes besides the pivot
LAYOUT_ENV = "MEMO_INDEX_DAP_LAYOUT"   # `memo index`: auto (unset) | dense | coded
BUDGET_ENV = "MEMO_INDEX_WALK_BUDGET"  # `memo index`: the walk's budget (unset: the library's default)
STATS_ENV = "MEMO_INDEX_STATS"         # `memo index`: a file that receives build_index's stats as one JSON line
LAYOUTS = {"auto": 0, "dense": 1, "coded": 2}          # MEMO_MS_LAYOUT_*
_LAYOUT_NAMES = {v: k for k, v in LAYOUTS.items()}


class FastaError(ValueError):
    """input that `memo index` refuses rather than index wrongly"""


def parse_fasta(data, path="<fasta>"):
    """[(name, sequence bytes)] of a FASTA file's bytes: name = first whitespace-delimited word after '>',
    sequence = the record's lines joined, all whitespace removed, upper-cased"""
    if data[:2] == b"\x1f\x8b":
        raise FastaError(f"{path}: gzip-compressed FASTA is not supported; decompress it first")
    if SEPARATOR in data:
        raise FastaError(f"{path}: holds a NUL byte")
    parts = (b"\n" + data).split(b"\n>")
    if parts[0].strip():
        raise FastaError(f"{path}: not FASTA (text before the first '>' header)")
    records = []
    for part in parts[1:]:
        header, _, body = part.partition(b"\n")
        words = header.split()
        name = words[0].decode("utf-8", "replace") if words else ""
        records.append((name, body.translate(None, _WHITESPACE).upper()))
    return records


def read_fasta(path):
    with open(path, "rb") as fh:
        return parse_fasta(fh.read(), path)


def revcomp(seq):
    """reverse complement as `samtools faidx -i` writes it"""
    return seq.translate(_COMPLEMENT)[::-1]


def genome_text(seqs):
    """S_1 $ ... S_s $ rc(S_1) $ ... rc(S_s) $ (index.sh:63-65), $ = NUL"""
    if not seqs:
        return b""
    return SEPARATOR.join(list(seqs) + [revcomp(s) for s in seqs]) + SEPARATOR


def pivot_layout(records, path="<pivot>"):
    """(names, concatenated bytes, int64 record offsets [nrec + 1]) -- what the .fai gave dap_to_bed.py"""
    if not records:
        raise FastaError(f"{path}: the pivot has no records")
    for name, seq in records:
        if not seq:
            raise FastaError(f"{path}: pivot record '{name}' has length 0")
        if len(seq) > MAX_RECORD:
            raise FastaError(f"{path}: pivot record '{name}' has {len(seq)} positions (the limit is {MAX_RECORD})")
    rec_begin = np.zeros(len(records) + 1, np.int64)
    rec_begin[1:] = np.cumsum([len(s) for _, s in records])
    return [n for n, _ in records], b"".join(s for _, s in records), rec_begin


class MatchingStatistics:
    """The DAP int32 [positions][columns] of one pivot, resident on `device` (memo_ms_*): as that matrix (layout "dense"),
    as run-coded columns ("coded"), or dense where the matrix fits in the free device memory and coded where not ("auto")"""

    def __init__(self, pivot, rec_begin, columns, device=0, chunk=0, layout="auto", walk_budget=None):
        self._h = C.c_void_p()
        self.rec_begin = np.ascontiguousarray(rec_begin, np.int64)
        self.positions = int(self.rec_begin[-1])
        self.columns = columns
        self._pivot = bytes(pivot)
        if len(self._pivot) != self.positions:
            raise ValueError(f"pivot has {len(self._pivot)} bytes, its records {self.positions}")
        check(lib().memo_ms_create_layout(self._pivot, self.rec_begin.ctypes.data, len(self.rec_begin) - 1, columns,
                                          int(chunk), device, _layout_number(layout), C.byref(self._h)))
        if walk_budget is not None:
            try:
                self.set_walk_budget(walk_budget)
            except BaseException:
                self.close()
                raise

    def set_walk_budget(self, steps):
        """the characters the walks of the adds to come extend a match one at a time before the rest is looked up by seed
        search: 0 seeds at once, 2^30 or more never, None or a negative value restores the default"""
        check(lib().memo_ms_set_walk_budget(self._h, -1 if steps is None else int(steps)))

    def walk_info(self):
        """{"text_reads", "max_chunk_text_reads", "seeds", "seed_text_reads", "budget"} of the last add's walks
        (memo_ms_walk_info; all zeros before the first add)"""
        from ._lib import MsWalkInfo
        info = MsWalkInfo()
        check(lib().memo_ms_walk_info(self._h, C.byref(info)))
        return {name: getattr(info, name) for name, _ in MsWalkInfo._fields_}

    def layout_info(self):
        """{"layout": "dense" | "coded", "block": positions per coding block, "device_bytes": held for the DAP now,
        "dense_bytes": what the matrix takes, "flagged": flagged positions of all columns, "encode_ms", "decode_ms"}"""
        from ._lib import MsLayoutInfo
        info = MsLayoutInfo()
        check(lib().memo_ms_layout_info(self._h, C.byref(info)))
        out = {name: getattr(info, name) for name, _ in MsLayoutInfo._fields_}
        out["layout"] = _LAYOUT_NAMES[info.layout]
        return out

    def column_info(self, column):
        """{"flagged", "bytes"} of one column (memo_ms_column_info)"""
        flagged, nbytes = C.c_uint64(), C.c_uint64()
        check(lib().memo_ms_column_info(self._h, column, C.byref(flagged), C.byref(nbytes)))
        return {"flagged": flagged.value, "bytes": nbytes.value}

    def add(self, text, column):
        """matching statistics of the pivot against one genome text, into DAP column `column`"""
        if len(text) > MAX_TEXT:
            raise MemoError(-1, f"genome text of {len(text)} bytes: the limit is {MAX_TEXT}")
        check(lib().memo_ms_add_genome(self._h, bytes(text), len(text), column))

    def add_records(self, seqs, column, piece_bytes=0):
        """matching statistics of the pivot against the genome whose records are `seqs` (list of bytes), into DAP
        column `column`: its text genome_text(seqs) is assembled on the device in pieces of at most `piece_bytes`
        bytes (<= 0: the library's default cap), of any total length; returns the number of pieces"""
        seqs = [bytes(s) for s in seqs]
        rec_begin = np.zeros(len(seqs) + 1, np.int64)
        rec_begin[1:] = np.cumsum([len(s) for s in seqs])
        pieces = C.c_int32()
        check(lib().memo_ms_add_records(self._h, b"".join(seqs), rec_begin.ctypes.data, len(seqs), column,
                                        int(piece_bytes), C.byref(pieces)))
        return pieces.value

    def fetch(self, first=0, positions=None):
        positions = self.positions - first if positions is None else positions
        out = np.empty((positions, self.columns), np.int32)
        check(lib().memo_ms_fetch(self._h, first, positions, out.ctypes.data))
        return out

    def timings(self):
        """device milliseconds so far: suffix arrays, LCP + hierarchy, MS walks"""
        t = (C.c_float * 3)()
        check(lib().memo_ms_timings(self._h, t))
        return {"sa_ms": t[0], "lcp_ms": t[1], "walk_ms": t[2]}

    def close(self):
        if self._h:
            lib().memo_ms_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def plan_pieces(lengths, cap):
    """(pieces, int32 piece of every string): memo_ms_add_records' plan for records of these lengths -- strings S_1 ..
    S_s, rc(S_1) .. rc(S_s) of len + 1 bytes each, greedily into pieces of at most `cap` bytes (host only)"""
    lengths = np.ascontiguousarray(lengths, np.int64)
    piece = np.zeros(2 * len(lengths), np.int32)
    pieces = C.c_int32()
    check(lib().memo_ms_plan_pieces(lengths.ctypes.data, len(lengths), int(cap), piece.ctypes.data, C.byref(pieces)))
    return pieces.value, piece


def _layout_number(layout):
    if layout not in LAYOUTS:
        raise ValueError(f"layout {layout!r}: need one of {', '.join(LAYOUTS)}")
    return LAYOUTS[layout]


def plan_layout(positions, columns, free_bytes, layout="auto"):
    """(layout name, bytes it needs at creation): memo_ms_create_layout's decision for a pivot of `positions` positions and
    `columns` columns with `free_bytes` of device memory free (host only); MemoError ("device memory") when nothing fits"""
    chosen, floor = C.c_int32(), C.c_int64()
    number = layout if isinstance(layout, int) else _layout_number(layout)
    check(lib().memo_ms_plan_layout(int(positions), int(columns), int(free_bytes), number, C.byref(chosen), C.byref(floor)))
    return _LAYOUT_NAMES[chosen.value], floor.value


def dap_layout_from_env(environ=os.environ):
    """the DAP layout MEMO_INDEX_DAP_LAYOUT asks for ("auto" when unset or empty); FastaError when it is none of auto, dense,
    coded (exactly so: no other case, no blanks)"""
    raw = environ.get(LAYOUT_ENV, "")
    if raw == "":
        return "auto"
    if raw not in LAYOUTS:
        raise FastaError(f"{LAYOUT_ENV}={raw!r}: need one of {', '.join(LAYOUTS)}")
    return raw


def piece_bytes_from_env(environ=os.environ):
    """the piece cap MEMO_INDEX_PIECE_BYTES asks for (0: unset, the library's default); FastaError when it is not an
    integer in [2, 2^31 - 2]"""
    raw = environ.get(PIECE_ENV, "")
    if raw == "":
        return 0
    try:
        cap = int(raw)
    except ValueError:
        cap = None
    if cap is None or not 2 <= cap <= MAX_TEXT:
        raise FastaError(f"{PIECE_ENV}={raw!r}: need an integer in [2, {MAX_TEXT}]")
    return cap


def walk_budget_from_env(environ=os.environ):
    """the walk budget MEMO_INDEX_WALK_BUDGET asks for (None: unset, the library's default); FastaError when it is not an
    integer >= 0 (decimal digits only: no sign, no blanks)"""
    raw = environ.get(BUDGET_ENV, "")
    if raw == "":
        return None
    if not (raw.isascii() and raw.isdigit()) or len(raw) > 18:
        raise FastaError(f"{BUDGET_ENV}={raw!r}: need an integer >= 0 (below 10^18)")
    return int(raw)


def matching_statistics(pivot, genomes, device=0, chunk=0):
    """MS matrix int32 [pivot positions][len(genomes)] of pivot records (list of bytes) against genomes (each a
    list of record bytes), by the rule in the module docstring"""
    _, seq, rec_begin = pivot_layout([(str(i), s) for i, s in enumerate(pivot)])
    with MatchingStatistics(seq, rec_begin, len(genomes), device, chunk) as ms:
        for c, recs in enumerate(genomes):
            ms.add(genome_text(recs), c)
        return ms.fetch()


def read_genome_list(path):
    if not path:
        raise FastaError("no genome list: give one with -g")
    try:
        with open(path) as fh:
            paths = [ln.strip() for ln in fh if ln.strip()]
    except OSError as exc:
        raise FastaError(f"cannot read the genome list {path}: {exc.strerror}") from None
    if len(paths) < 2:
        raise FastaError(f"{path}: needs the pivot and at least one more genome")
    if len(paths) - 1 > MAX_COLUMNS:
        raise FastaError(f"{path}: {len(paths) - 1} genomes besides the pivot (the limit is {MAX_COLUMNS})")
    return paths


def build_index(genome_list, out_dir, prefix, membership, device=0, chunk=0, log=print, keep_ms=False, piece_bytes=0,
                layout="auto", walk_budget=None):
    """index.sh end to end; returns per-stage seconds, the pieces of every genome's text (and the MS matrix when
    keep_ms).  piece_bytes: the cap of a piece of genome text (<= 0: the library's default).  layout: of the DAP on the
    device, "auto" | "dense" | "coded" (stats: dap_layout, the one taken; dap_device_bytes, held for the DAP after the last
    genome; per genome, flagged: its column's flagged positions, 0 in the dense layout).  walk_budget: MatchingStatistics' (None: the
    default; stats: walk_budget, the one taken; per genome, seeds and max_chunk_text_reads of its walks).  Row batches go to the Parquet writer
    as they are produced (each is written and dropped before the next is made), so the two stages interleave: dap_to_rows_s
    is the time spent making batches, parquet_s the rest of that one loop."""
    from .dap_to_bed import DapConverter, write_parquet
    t0 = time.perf_counter()
    paths = read_genome_list(genome_list)
    _layout_number(layout)
    names, pivot, rec_begin = pivot_layout(read_fasta(paths[0]), paths[0])
    stats = {"positions": int(rec_begin[-1]), "genomes": len(paths), "read_s": 0.0, "pieces": [], "per_genome": [],
             "walk_budget": None}         # (the budget of the walks: no walk, no budget)
    stats["read_s"] += time.perf_counter() - t0
    out_path = os.path.join(out_dir, prefix + ".parquet")
    os.makedirs(out_dir or ".", exist_ok=True)
    with MatchingStatistics(pivot, rec_begin, len(paths) - 1, device, chunk, layout, walk_budget) as ms:
        stats["dap_layout"] = ms.layout_info()["layout"]
        t1 = time.perf_counter()
        for c, path in enumerate(paths[1:]):
            tr = time.perf_counter()
            records = read_fasta(path)
            read_s = time.perf_counter() - tr
            stats["read_s"] += read_s
            log(f"Finding MS between pivot and {os.path.basename(path)}")
            before = ms.timings()
            try:
                stats["pieces"].append(ms.add_records([s for _, s in records], c, piece_bytes))
            except MemoError as exc:
                m = re.search(r"genome record (\d+) ", str(exc))
                if not m:
                    raise
                raise FastaError(f"{path}: record '{records[int(m.group(1))][0]}': {exc}") from None
            after = ms.timings()
            walk = ms.walk_info()
            stats["walk_budget"] = walk["budget"]
            stats["per_genome"].append({"bases": sum(len(s) for _, s in records), "records": len(records),
                                        "pieces": stats["pieces"][-1], "read_s": read_s,
                                        "flagged": ms.column_info(c)["flagged"],
                                        "seeds": walk["seeds"], "max_chunk_text_reads": walk["max_chunk_text_reads"],
                                        **{k: after[k] - before[k] for k in after}})
            del records
        stats["ms_s"] = time.perf_counter() - t1
        stats.update(ms.timings())
        info = ms.layout_info()
        stats["dap_device_bytes"] = info["device_bytes"]
        stats["encode_ms"] = info["encode_ms"]
        if keep_ms:
            stats["ms"] = ms.fetch()
        log("Making membership index" if membership else "Making conservation index")
        t2 = time.perf_counter()
        npos, C_ = ms.positions, ms.columns
        block = max(1024, (64 << 20) // C_)
        made = [0.0]

        def batches():
            """every row batch once: written and dropped before the next is made"""
            with DapConverter(C_, rec_begin, not membership, True, device) as conv:
                for first in range(0, npos, block):
                    tb = time.perf_counter()
                    b = conv.push_ms(ms, first, min(block, npos - first))
                    made[0] += time.perf_counter() - tb
                    yield names, b
                tb = time.perf_counter()
                b = conv.finish()
                made[0] += time.perf_counter() - tb
                yield names, b
        log("Compressing index.")
        part_path = out_path + ".part"           # a failure while rows are made or written leaves no index behind
        try:
            rows = write_parquet(part_path, batches())
            os.replace(part_path, out_path)
        except BaseException:
            if os.path.exists(part_path):
                os.unlink(part_path)
            raise
        stats["decode_ms"] = ms.layout_info()["decode_ms"]
        stats["dap_to_rows_s"] = made[0]
        stats["parquet_s"] = time.perf_counter() - t2 - made[0]
    stats["rows"] = rows
    stats["total_s"] = time.perf_counter() - t0
    log("DONE")
    return stats


def main(argv):
    """bin/memo index [options]; exit statuses and usage handling of index.sh"""
    if not argv or argv[0] == "-h":
        sys.stdout.write(USAGE)
        sys.exit(0)
    try:
        opts, _ = getopt.getopt(argv, "g:o:p:m")
    except getopt.GetoptError as exc:               # bash getopts: message on stderr, then usage, exit 0
        what = "option requires an argument" if "requires argument" in exc.msg else "illegal option"
        sys.stderr.write(f"{sys.argv[0]}: {what} -- {exc.opt}\n")
        sys.stdout.write(USAGE)
        sys.exit(0)
    val = {"-o": "."}                                # index.sh:6
    for o, a in opts:
        val[o] = a
    try:
        if not val.get("-p"):
            raise FastaError("no output prefix: give one with -p")
        read_genome_list(val.get("-g", ""))          # refuse before the device is touched
        piece_bytes = piece_bytes_from_env()
        layout = dap_layout_from_env()
        walk_budget = walk_budget_from_env()
        stats = build_index(val["-g"], val["-o"], val["-p"], "-m" in val, int(os.environ.get("MEMO_DEVICE", "0")),
                            log=lambda s: print(s, flush=True), piece_bytes=piece_bytes, layout=layout,
                            walk_budget=walk_budget)
        if os.environ.get(STATS_ENV):
            import json
            with open(os.environ[STATS_ENV], "w") as fh:
                fh.write(json.dumps(stats) + "\n")
    except (FastaError, MemoError) as exc:
        sys.stderr.write(f"memo index: {exc}\n")
        sys.exit(1)


if __name__ == "__main__":
    main(sys.argv[1:])
