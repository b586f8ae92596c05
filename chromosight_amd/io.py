""".cool ingestion for the device pipeline: the HDF5 datasets the reference
reads through cooler (contacts_map.py:129, 209, 529: pixel table, bin table with ICE weights,
chromosome offsets) decoded into the dictionary `pipeline.DeviceCool` uploads.

Neither cooler nor h5py exists in the target image, and the path needs nothing of them: a .cool is a
handful of 1-D HDF5 datasets.  They are decoded by chromosight_amd.hdf5_lite (numpy + zlib: the classic
HDF5 format h5py writes by default); files in a newer format fall back to the HDF5 command line tool
`h5dump -b` (located through $CHROMOSIGHT_H5DUMP, PATH or /opt/conda/bin).  Multi-resolution files:
`path::/resolutions/2000`.
"""
import csv
import json
import os
import pathlib
import re
import shutil
import subprocess
import tempfile

import numpy as np

from . import hdf5_lite

_TYPES = {"H5T_STD_I8LE": "<i1", "H5T_STD_I16LE": "<i2", "H5T_STD_I32LE": "<i4", "H5T_STD_I64LE": "<i8",
          "H5T_STD_U8LE": "<u1", "H5T_STD_U16LE": "<u2", "H5T_STD_U32LE": "<u4", "H5T_STD_U64LE": "<u8",
          "H5T_IEEE_F32LE": "<f4", "H5T_IEEE_F64LE": "<f8"}


def find_h5dump():
    for cand in (os.environ.get("CHROMOSIGHT_H5DUMP"), shutil.which("h5dump"), "/opt/conda/bin/h5dump",
                 "/usr/bin/h5dump"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("no h5dump found (set CHROMOSIGHT_H5DUMP): .cool files are decoded with the HDF5 "
                       "command line tools; alternatively pass an already decoded pixel table (dict / npz)")


def _run(args):
    return subprocess.run(args, check=True, capture_output=True, text=True).stdout


def _header(tool, path, dataset):
    txt = _run([tool, "-H", "-d", dataset, str(path)])
    head = txt[:txt.index("DATASPACE")]
    m = re.search(r"DATATYPE\s+(H5T_\w+)", head)
    enum = re.search(r"H5T_ENUM\s*{\s*(H5T_\w+);", head)
    return (enum.group(1) if enum else m.group(1)), head


def _numeric(tool, path, dataset):
    kind, _ = _header(tool, path, dataset)
    if kind not in _TYPES:
        raise ValueError(f"{dataset}: unsupported HDF5 type {kind}")
    with tempfile.TemporaryDirectory() as tmp:
        out = pathlib.Path(tmp) / "d.bin"
        subprocess.run([tool, "-d", dataset, "-b", "LE", "-o", str(out), str(path)], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return np.fromfile(out, dtype=_TYPES[kind])


def _strings(tool, path, dataset):
    txt = _run([tool, "-d", dataset, str(path)])
    data = txt[txt.index("DATA {"):]
    return [x.split("\\000")[0] for x in re.findall(r'"([^"]*)"', data)]


def _attr_int(tool, path, group, name):
    txt = _run([tool, "-a", f"{group}/{name}".replace("//", "/"), str(path)])
    return int(re.search(r"\(0\):\s*(-?\d+)", txt).group(1))


def _weights(uri, balance, norm, n_bins, read):
    """The balancing weights under the rules of load_cool; read() returns the column or None when it is absent."""
    weight = read()
    if norm is None:                      # _read_cool: the column as stored, None when the file has none
        return None if weight is None else np.asarray(weight, dtype=np.float64)
    if weight is not None:
        weight = np.asarray(weight, dtype=np.float64)
        return np.where(np.isfinite(weight), 1.0, np.nan) if norm == "raw" else weight
    if norm == "raw":
        return np.ones(n_bins)
    raise ValueError(f"{uri}: no balancing weights (bins/{balance}).  Balance the file first (cooler balance; the "
                     "reference does it with cooler.balance_cooler) or pass norm='raw' to scan raw counts with every "
                     "bin detectable")


def _load_cool_native(path, group, balance, norm):
    """load_cool through chromosight_amd.hdf5_lite (no external tool)."""
    with hdf5_lite.File(path) as f:                       # (closes the mapping and the handle: ADVICE r3)
        return _read_cool_datasets(f, path, group, balance, norm)


def _read_cool_geometry(f, path, group, balance, norm):
    """Everything of a .cool but its pixel table: names, offsets, bin starts / ends, bin size and the weights under _weights' rules."""
    ds = lambda name: f"{group}/{name}"
    names = f.dataset(ds("chroms/name"))
    attrs = f.attrs(group or "/")
    if "bin-size" not in attrs:
        raise hdf5_lite.Hdf5Unsupported("no numeric bin-size attribute (variable-size bins?)")
    cool = {
        "bin_start": f.dataset(ds("bins/start")).astype(np.int64),
        "bin_end": f.dataset(ds("bins/end")).astype(np.int64),
        "chrom_offset": f.dataset(ds("indexes/chrom_offset")).astype(np.int64),
        "chrom_names": np.array([n.split(b"\0")[0].decode() for n in names]),
        "binsize": np.int64(attrs["bin-size"]),
    }
    cool["weight"] = _weights(path, balance, norm, cool["bin_start"].size,
                              lambda: f.dataset(ds(f"bins/{balance}")) if f.exists(ds(f"bins/{balance}")) else None)
    return cool


def _read_cool_datasets(f, path, group, balance, norm):
    ds = lambda name: f"{group}/{name}"
    cool = {
        "bin1_id": f.dataset(ds("pixels/bin1_id")),
        "bin2_id": f.dataset(ds("pixels/bin2_id")),
        "count": f.dataset(ds("pixels/count")),
    }
    cool.update(_read_cool_geometry(f, path, group, balance, norm))
    return cool


def _has_dataset(tool, path, dataset):
    """Is `dataset` an object of the file?  (`h5dump -n` lists every group and dataset.)"""
    listing = _run([tool, "-n", str(path)])
    return re.search(r"^\s*dataset\s+" + re.escape(dataset) + r"\s*$", listing, flags=re.M) is not None


def _load_cool_h5dump(uri, path, group, balance, norm):
    """load_cool through the HDF5 command line tool (`h5dump -b`: any chunking, compression, format version)."""
    tool = find_h5dump()
    ds = lambda name: f"{group}/{name}"
    n_bins = None
    cool = {
        "bin1_id": _numeric(tool, path, ds("pixels/bin1_id")),
        "bin2_id": _numeric(tool, path, ds("pixels/bin2_id")),
        "count": _numeric(tool, path, ds("pixels/count")),
        "bin_start": _numeric(tool, path, ds("bins/start")).astype(np.int64),
        "bin_end": _numeric(tool, path, ds("bins/end")).astype(np.int64),
        "chrom_offset": _numeric(tool, path, ds("indexes/chrom_offset")).astype(np.int64),
        "chrom_names": np.array(_strings(tool, path, ds("chroms/name"))),
        "binsize": np.int64(_attr_int(tool, path, group or "/", "bin-size")),
    }
    n_bins = cool["bin_start"].size
    cool["weight"] = _weights(uri, balance, norm, n_bins,
                              lambda: _numeric(tool, path, ds(f"bins/{balance}")) if _has_dataset(tool, path, ds(f"bins/{balance}")) else None)
    return cool


def load_cool(uri, balance="weight", norm="auto"):
    """Decode a .cool (or `file.mcool::/resolutions/<binsize>`) into the dictionary of arrays the
    device pipeline takes: bin1_id, bin2_id, count, weight (NaN = bin without a balancing weight),
    bin_start, bin_end, chrom_offset, chrom_names, binsize.  The pixel table comes back in the file's
    order (cooler: sorted by bin1, bin2).

    The file must be balanced: the reference balances an unbalanced file itself (cooler.balance_cooler,
    contacts_map.py:203-221) and ALWAYS takes the detectable bins from the finite weights (:227); ICE balancing is
    outside this package, so a file without a `bins/<balance>` column is refused (ValueError) instead of being
    scanned as raw counts with every bin detectable.  norm="raw" is the explicit opt-in for exactly that
    (all-ones weights; the reference's --norm raw still balances first to find the detectable bins, so results on
    an unbalanced file differ from it in the bins it would have masked).  Read errors of an existing weight
    column (h5dump failure, unsupported type) propagate."""
    if norm not in ("auto", "raw"):
        raise ValueError("norm must be one of: auto, raw ('force' re-balances the file: not part of this package)")
    return _load(uri, balance, norm)


def _read_cool(uri, balance="weight"):
    """The dictionary of load_cool with the `bins/<balance>` column exactly as stored, or weight None when the file has no
    such column (pipeline.open_cool balances it on the device).  Never writes to the file."""
    return _load(uri, balance, None)


def split_uri(uri):
    """(path, group) of `file.cool` or `file.mcool::/resolutions/<binsize>`."""
    path, _, group = str(uri).partition("::")
    return path, "/" + group.strip("/") if group else ""


def _load(uri, balance, norm):
    path, group = split_uri(uri)
    cool = None
    if not os.environ.get("CHROMOSIGHT_H5DUMP_ONLY"):
        try:
            cool = _load_cool_native(path, group, balance, norm)
        except hdf5_lite.Hdf5Unsupported:
            cool = None                  # a file written with a newer HDF5 format: the command line tool below
    if cool is None:
        cool = _load_cool_h5dump(uri, path, group, balance, norm)
    for key in ("bin1_id", "bin2_id"):
        if cool[key].size and cool[key].max() < 2 ** 31:
            cool[key] = cool[key].astype(np.int32)
    return cool


# ------------------------------------------------------------------------------------------------
# output side of `detect` / `quantify`: the files the reference writes
# ------------------------------------------------------------------------------------------------
def check_prefix_dir(prefix):
    """The parent directory of an output prefix must exist (reference io.py:338-342: OSError)."""
    parent = os.path.dirname(prefix)
    if parent and not os.path.isdir(parent):
        raise OSError(f"Directory {parent} does not exist.")


def write_patterns(coords, output_prefix, dec=10):
    """<prefix>.tsv of a pattern table (reference io.py:208-226): tab separated, no index, floats with
    `dec` decimals -- byte-comparable with the reference's output for the same table."""
    coords.to_csv(output_prefix + ".tsv", sep="\t", index=False, float_format=f"%.{int(dec)}f")


def save_windows(windows, output_prefix, fmt="json"):
    """The windows around the patterns, stacked on axis 0 (reference io.py:229-256): <prefix>.npy, or
    <prefix>.json = {"0": [[...]], "1": ...} (NaN written as NaN, as json.dump does)."""
    windows = np.asarray(windows)
    if fmt == "npy":
        np.save(output_prefix + ".npy", windows)
    elif fmt == "json":
        with open(output_prefix + ".json", "w") as handle:
            json.dump({k: w.tolist() for k, w in enumerate(windows)}, handle, indent=4)
    else:
        raise ValueError("window format must be either npy or json.")


BED2D_COLUMNS = ["chrom1", "start1", "end1", "chrom2", "start2", "end2"]


def load_bed2d(path):
    """First six columns of a 2-D BED file as a DataFrame (reference io.py:284-326): a header line is
    detected (csv.Sniffer, like the reference) or the standard names are given; chromosome names are
    strings; intra-chromosomal pairs are oriented so that anchor 1 is the left one.  Reads the output of
    `detect` as the input of `quantify`."""
    import pandas as pd
    with open(path) as handle:
        has_header = csv.Sniffer().has_header(handle.read(65536))
    if has_header:
        bed = pd.read_csv(path, sep="\t", header=0, usecols=range(6))
    else:
        bed = pd.read_csv(path, sep="\t", header=None, names=BED2D_COLUMNS, usecols=range(6))
    bed = bed.copy()
    c1, c2 = bed.columns[0], bed.columns[3]
    bed[c1] = bed[c1].astype(str)
    bed[c2] = bed[c2].astype(str)
    s1, e1, s2, e2 = bed.columns[1], bed.columns[2], bed.columns[4], bed.columns[5]
    flip = ((bed[s2] < bed[s1]) & (bed[c1] == bed[c2])).to_numpy()
    if flip.any():
        a = bed.loc[flip, [s1, e1]].to_numpy()
        b = bed.loc[flip, [s2, e2]].to_numpy()
        bed.loc[flip, [s1, e1]] = b
        bed.loc[flip, [s2, e2]] = a
    return bed


PAIRS_COLUMNS = ("chr1", "pos1", "chr2", "pos2")


class PairsFile:
    """A 4DN .pairs text file (plain or .gz) as a stream of chunks for cload.pairs_device: what read_pairs returns.  The header is
    read when the object is made (`chromsizes`: the #chromsize: lines or the caller's; `columns`: the 0-based fields of chr1, pos1,
    chr2, pos2); iterating reads the body, `chunk_rows` lines at a time, and yields (chrom1, pos1, chrom2, pos2) arrays: int32 ids
    into `chromsizes` (-1: a name that is not in it) and int64 positions as the file has them (1-based in this format)."""

    def __init__(self, path, chromsizes=None, chunk_rows=1 << 24):
        if isinstance(chunk_rows, bool) or int(chunk_rows) != chunk_rows or int(chunk_rows) < 1:
            raise ValueError(f"chunk_rows must be a positive integer, got {chunk_rows!r}")
        self.path = os.fspath(path)
        self.chunk_rows = int(chunk_rows)
        header_sizes, columns, self.header_lines, self.width = {}, None, 0, 0
        with self._open() as handle:
            for line in handle:
                if not line.startswith("#"):
                    self.width = len(line.rstrip("\r\n").split("\t")) if line.strip() else 0
                    break
                self.header_lines += 1
                fields = line.split()
                if fields and fields[0] == "#chromsize:":
                    if len(fields) != 3:
                        raise ValueError(f"{self.path}, line {self.header_lines}: a #chromsize: line holds a name and a length")
                    header_sizes[fields[1]] = int(fields[2])
                elif fields and fields[0] == "#columns:":
                    columns = fields[1:]
        if columns is None:
            self.columns = (1, 2, 3, 4)             # readID chr1 pos1 chr2 pos2 ...: fields 2 to 5
        else:
            missing = [name for name in PAIRS_COLUMNS if name not in columns]
            if missing:
                raise ValueError(f"{self.path}: the #columns: line names no {', '.join(missing)}")
            self.columns = tuple(columns.index(name) for name in PAIRS_COLUMNS)
        if chromsizes is None:
            if not header_sizes:
                raise ValueError(f"{self.path} has no #chromsize: lines: pass chromsizes")
            chromsizes = header_sizes
        items = list(chromsizes.items()) if hasattr(chromsizes, "items") else [tuple(x) for x in chromsizes]
        self.chromsizes = {str(name): int(length) for name, length in items}

    def _open(self):
        if self.path.endswith(".gz"):
            import gzip
            return gzip.open(self.path, "rt")
        return open(self.path, "rt")

    def _short_line(self):
        """ValueError for the first body line with too few fields (a walk in Python: only on the way to an error), or None."""
        need = max(self.columns) + 1
        with self._open() as handle:
            for k, line in enumerate(handle):
                if k >= self.header_lines and len(line.rstrip("\r\n").split("\t")) < need:
                    return ValueError(f"{self.path}, line {k + 1}: too few fields for the columns {', '.join(PAIRS_COLUMNS)}")
        return None

    def __iter__(self):
        import pandas as pd
        if self.width <= max(self.columns):                   # the first body line is short, or there is no body
            error = self._short_line()
            if error is not None:
                raise error
            return
        names = list(self.chromsizes)
        line = self.header_lines                              # lines in front of the chunk at hand
        with self._open() as handle:
            reader = pd.read_csv(handle, sep="\t", header=None, names=list(range(self.width)), usecols=sorted(set(self.columns)),
                                 skiprows=self.header_lines, dtype=str, na_filter=False, skip_blank_lines=False, comment=None,
                                 quoting=csv.QUOTE_NONE, chunksize=self.chunk_rows)
            while True:
                try:
                    frame = next(reader)
                except StopIteration:
                    return
                except pd.errors.ParserError:                 # (a chunk of short lines only, for one)
                    error = self._short_line()
                    if error is None:
                        raise
                    raise error from None
                cols = [frame[c].to_numpy() for c in self.columns]
                if any((col == "").any() for col in cols):
                    raise self._short_line() or ValueError(f"{self.path}, lines {line + 1} to {line + len(frame)}: an empty field")
                ids = [pd.Categorical(cols[k], categories=names).codes.astype(np.int32) for k in (0, 2)]
                try:
                    pos = [cols[k].astype(np.int64) for k in (1, 3)]
                except (ValueError, OverflowError):
                    raise ValueError(f"{self.path}, lines {line + 1} to {line + len(frame)}: a position that is not an integer") from None
                line += len(frame)
                yield ids[0], pos[0], ids[1], pos[1]


def read_pairs(path, chromsizes=None, chunk_rows=1 << 24):
    """A host reader of the 4DN .pairs text format (what pairtools writes), plain or .gz: a PairsFile.  #chromsize: header lines
    give `chromsizes` when the caller passes none (ValueError when there are none either); a #columns: line locates chr1 / pos1 /
    chr2 / pos2 (default: fields 2 to 5); the body is tab-separated.  Iterating yields chunks of at most `chunk_rows` pairs as
    (chrom1, pos1, chrom2, pos2) arrays with the names mapped to ids on the host, -1 for a name that is not in `chromsizes`.  A
    line with too few fields raises ValueError with its line number."""
    return PairsFile(path, chromsizes, chunk_rows)
