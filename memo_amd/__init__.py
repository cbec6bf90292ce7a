"""memo_amd -- MI355X-native implementation of MEMO's windowed k-mer query path.

Layout (only what the path needs):
  csrc/            HIP kernels for gfx950 + the C ABI (include/memo_amd*.h)
  _lib.py          ctypes binding of libmemo_amd.so -- raises if the library is missing
  _device.py       for the drivers below: DevBuffer, the one owner of a device allocation; RowBuffer; on_device; emit_text
  _window.py       for the drivers below: parse_region (CHR:START-END), membership_slices (a window swept slice by slice)
  _cli.py          for the NAME_cli.py below: usage, refusals, the flags, the device, the error tail, the output file
  index.py         DeviceIndex: an index chromosome resident in HBM; IndexBuilder; sweep launches
  memo_query.py    host-side mirror of the reference's src/memo_query.py (same function
                   names and argument meaning: filter_pq, memo_init, memo_query, print_res)
  cache.py         sidecar cache of a record's packed rows next to the Parquet index
  _fastquery.py    `memo query` answered from that cache with nothing but ctypes (no NumPy import)
  synth.py         the synthetic pangenome workloads of BASELINE.json
  shard.py         window sharding across ranks + gather (torch.distributed)
  dap_to_bed.py    DAP -> index rows on the GPU -> BED text or Parquet
  build_index.py   `memo index`: FASTA genomes -> matching statistics on the GPU -> Parquet index
  view.py          `memo view` preprocessing: result text parsed and binned on the GPU, or a window binned from an index
  view_cli.py      `memo view`: flags, usage, the table as TSV, the plot (matplotlib)
  regions.py       `memo regions`: a result's runs of equal value compacted on the GPU, a window's runs from an index
  regions_cli.py   `memo regions`: flags, usage, bedGraph / BED3 / BED + membership string
  matrix.py        `memo matrix`: a membership result's co-occurrence matrix counted on the GPU, a window's in slices
  matrix_cli.py    `memo matrix`: flags, usage, counts or Jaccard distances as tab-separated text
  collect.py       `memo collect`: core and covered k-mer curves over genome orders, reduced on the GPU, a window's in slices
  collect_cli.py   `memo collect`: flags, usage, the curve, the band over random orders or every order as tab-separated text
  panel.py         `memo panel`: the greedy set cover of a window's membership bits, on per-genome bit planes that stay on the GPU
  panel_cli.py     `memo panel`: flags, usage, the curve of the chosen order with the genome each line adds
  cover.py         `memo cover`: `memo panel` summed over every k, the greedy choice on per-genome weight planes that stay on the GPU
  cover_cli.py     `memo cover`: flags, usage, the curve of the chosen order over every k with the genome each line adds
  tracks.py        `memo tracks`: every genome's k-mer presence per bin along the pivot, counted on the GPU, a window's in slices
  tracks_cli.py    `memo tracks`: flags, usage, counts or fractions as tab-separated text, or the heat map (matplotlib)
  features.py      `memo features`: a BED file's features from one sweep per record: counted per segment, summed per feature on the GPU
  features_cli.py  `memo features`: flags, usage, counts, fractions or presence calls per feature as tab-separated text
  maxk.py          `memo maxk`: the longest shared k per position, all k in one pass over the rows, a window's from a Parquet index
  maxk_cli.py      `memo maxk`: flags, usage, one integer per line
  lengths.py       `memo lengths`: every genome's match length per position from a membership index, and the T-th largest, in slices
  lengths_cli.py   `memo lengths`: flags, usage, one integer per line or one per genome and line
  mems.py          `memo mems`: the maximal shared matches that start in a window, compacted on the GPU from the lengths where they lie
  mems_cli.py      `memo mems`: flags, usage, one interval per line
  breaks.py        `memo breaks`: match starts and length sums per genome and bin, or per BED feature, counted on the GPU where the lengths lie
  breaks_cli.py    `memo breaks`: flags, usage, counts, sums or their means as tab-separated text
  pairs.py         `memo pairs`: every pair of genomes' shared match length over a window, reduced on the GPU where the lengths lie
  pairs_cli.py     `memo pairs`: flags, usage, sums, weighted Jaccard distances or mean lengths as tab-separated text
  nearest.py       `memo nearest`: which genome matches the pivot longest, per genome and bin or as runs of the winner, reduced across the planes on the GPU
  nearest_cli.py   `memo nearest`: flags, usage, wins, sole wins or their shares as tab-separated text, or one interval per run of the winner
  mosaic.py        `memo mosaic`: the pivot as the fewest pieces copied whole from one genome each, the greedy parse by longest match, on the GPU
  mosaic_cli.py    `memo mosaic`: flags, usage, one interval per piece or the pieces' bases per genome and bin as tab-separated text
  spectrum.py      `memo spectrum`: a window's conservation histogram at every k from either kind of index, reduced on the GPU, in slices
  spectrum_cli.py  `memo spectrum`: flags, usage, the table as tab-separated text
  convert.py       `memo convert`: a membership index's lengths fed to the row builder: the conservation index, or the canonical membership index
  convert_cli.py   `memo convert`: flags, usage, the Parquet index written beside its name and renamed
  add.py           `memo add`: new genomes' matching statistics beside a membership index's lengths, fed to the row builder once
  add_cli.py       `memo add`: flags, usage, the grown membership and conservation indexes written beside their names and renamed
  merge.py         `memo merge`: the lengths of chosen genomes of one or more membership indexes on one pivot, fed to the row builder once
  merge_cli.py     `memo merge`: flags (per input and for the outputs), usage, the indexes and the genome list written beside their names

Attributes are loaded on first use (PEP 562), so that `import memo_amd._fastquery` -- the CLI's cache-hit
path -- does not pay for NumPy.
"""
__version__ = "0.2.0"

_LAZY = {
    "MemoError": "_lib", "MemoUnpackable": "_lib", "build": "_lib", "lib": "_lib",
    "DeviceIndex": "index", "IndexBuilder": "index", "conservation": "index", "membership": "index",
    "conservation_rows": "index", "membership_rows": "index",
    "emit_conservation": "index", "emit_membership": "index",
    "runs": "regions", "membership_runs": "regions", "region_runs": "regions",
    "cooccurrence": "matrix", "region_matrix": "matrix",
    "region_curves": "collect",
    "region_panel": "panel", "index_panel": "panel",
    "region_cover": "cover",
    "bin_tracks": "tracks", "region_tracks": "tracks",
    "bed_features": "features", "read_bed": "features",
    "region_maxk": "maxk", "index_maxk": "maxk",          # (maxk.maxk keeps its module's name: memo_amd.maxk is the module)
    "region_planes": "lengths", "region_kth": "lengths",
    "region_mems": "mems",
    "region_breaks": "breaks", "bed_breaks": "breaks", "plane_breaks": "breaks",
    "region_pairs": "pairs", "plane_sums": "pairs",
    "region_nearest": "nearest", "region_winners": "nearest", "plane_nearest": "nearest",
    "region_mosaic": "mosaic", "plane_mosaic": "mosaic", "bin_phrases": "mosaic",
    "region_exact": "spectrum",
    "convert_index": "convert",
    "add_index": "add",
    "merge_index": "merge",
}


def __getattr__(name):
    import importlib
    if name in _LAZY:
        value = getattr(importlib.import_module("." + _LAZY[name], __name__), name)
        globals()[name] = value
        return value
    if name in ("_lib", "_device", "_window", "_cli", "index", "memo_query", "cache", "synth", "shard", "view", "view_cli", "regions", "regions_cli", "matrix", "matrix_cli", "collect", "collect_cli", "panel", "panel_cli", "cover", "cover_cli", "tracks", "tracks_cli", "features", "features_cli", "maxk", "maxk_cli", "lengths", "lengths_cli", "mems", "mems_cli", "breaks", "breaks_cli", "pairs", "pairs_cli", "nearest", "nearest_cli", "mosaic", "mosaic_cli", "spectrum", "spectrum_cli", "convert", "convert_cli", "add", "add_cli", "merge", "merge_cli", "dap_to_bed", "build_index", "_fastquery"):
        return importlib.import_module("." + name, __name__)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def __dir__():
    return sorted(list(globals()) + list(_LAZY))
