"""What the tests of the device .pairs parser share (cs_pairs_text_parse, chromosight_amd/cload.py parse_pairs_text): a seeded
writer of .pairs text from columns, the flagged-line families, a plain Python restatement of the accepted grammar
(include/chromosight_hip.h) that says what the parser must answer for any text, and the record file of tools/pairs_text_check.cpp.
The restatement is itself held to the host reader (io.read_pairs) in tests/test_pairs_text_host.py; the judge of a table is always
the host route."""
import struct

import numpy as np

MAX_LINE = 65536            # asserted against cs_pairs_text_max_line_bytes() where a library is at hand
REASONS = {"empty_line": 1, "too_few": 2, "too_many": 3, "empty_field": 4, "bad_position": 5, "lone_cr": 6, "nul": 7, "high": 8,
           "too_long": 9}

# name -> (the 0-based fields of chr1, pos1, chr2, pos2; fields per line; the names of a #columns: line, or None for the default)
LAYOUTS = {
    "default": ((1, 2, 3, 4), 7, None),
    "late": ((9, 8, 7, 6), 10, "f0 f1 f2 f3 f4 f5 pos2 chr2 pos1 chr1".split()),
    "last": ((2, 3, 4, 5), 6, "readID x chr1 pos1 chr2 pos2".split()),
    "bare": ((0, 1, 2, 3), 4, "chr1 pos1 chr2 pos2".split()),
}


def header(chromsizes, layout="default", eol="\n"):
    """The header lines of a file over `chromsizes` (pairs of name and length) in `layout`, as text."""
    names = LAYOUTS[layout][2]
    lines = ["## pairs format v1.0"] + [f"#chromsize: {n} {s}" for n, s in chromsizes]
    if names is not None:
        lines.append("#columns: " + " ".join(names))
    return "".join(line + eol for line in lines)


def fields_of(layout, name1, pos1, name2, pos2, fill=".", n_fields=None):
    """The fields of one line (strings): the four values where `layout` has them, `fill` elsewhere -- a pair (first, rest) fills the
    first filler field with one string and the others with another; n_fields cuts the line short."""
    cols, width, _ = LAYOUTS[layout]
    first, rest = fill if isinstance(fill, tuple) else (fill, fill)
    out = [rest] * width
    spare = [k for k in range(width) if k not in cols]
    if spare:
        out[spare[0]] = first
    for c, v in zip(cols, (name1, pos1, name2, pos2)):
        out[c] = str(v)
    return out[:n_fields]


def body(names, chrom1, pos1, chrom2, pos2, layout="default", eol="\n", final=True, fill=".", fills=None, short=None):
    """The body text (bytes) of the pairs (name indices into `names`, positions) in `layout`: lines end with `eol`, the last one only
    when `final`; fills[i] replaces `fill` on line i (the way to place line ends); short: {line: number of fields} cuts lines."""
    lines = []
    for i in range(len(chrom1)):
        f = fill if fills is None or i >= len(fills) or fills[i] is None else fills[i]
        lines.append("\t".join(fields_of(layout, names[chrom1[i]], int(pos1[i]), names[chrom2[i]], int(pos2[i]), f,
                                         None if short is None else short.get(i))))
    text = eol.join(lines) + (eol if final and lines else "")
    return text.encode("ascii")


def random_columns(rng, n, n_names):
    """n seeded pairs: name indices below n_names and positions of 1 to 18 digits."""
    digits = rng.integers(1, 19, size=(2, n))
    pos = [np.asarray([int(rng.integers(10 ** (d - 1) if d > 1 else 0, 10 ** d)) for d in row], dtype=np.int64) for row in digits]
    return (rng.integers(0, n_names, size=n).astype(np.int32), pos[0], rng.integers(0, n_names, size=n).astype(np.int32), pos[1])


def fixed_length_body(names, chrom1, pos1, chrom2, pos2, length, layout="default", eol="\n"):
    """body() with every line, terminator included, exactly `length` bytes long: the first filler field makes up the difference."""
    fills = []
    for i in range(len(chrom1)):
        bare = "\t".join(fields_of(layout, names[chrom1[i]], int(pos1[i]), names[chrom2[i]], int(pos2[i]), ("", ".")))
        assert length - len(bare) - len(eol) >= 1, "the line does not fit"
        fills.append(("r" * (length - len(bare) - len(eol)), "."))
    return body(names, chrom1, pos1, chrom2, pos2, layout=layout, eol=eol, fills=fills)


def host_columns(directory, chromsizes, text, layout="default", tag="t"):
    """The columns io.read_pairs gives for the body `text` (bytes) behind the header of `layout`, and the file's path."""
    from chromosight_amd import io as cio
    path = directory / f"{tag}.pairs"
    path.write_bytes(header(chromsizes, layout).encode() + text)
    chunks = list(cio.read_pairs(path))
    if not chunks:
        return tuple(np.zeros(0, dtype=dt) for dt in (np.int32, np.int64, np.int32, np.int64)), path
    return tuple(np.concatenate([c[k] for c in chunks]) for k in range(4)), path


# ---- the flagged families: one valid line's fields -> the bytes of a line the device must flag (without terminator) ----------------
def _join(fields):
    return "\t".join(fields).encode("ascii")


def _with(fields, col, value):
    out = list(fields)
    out[col] = value
    return out


def flagged_line(family, layout, fields):
    """(bytes of the line without its terminator, reason code).  fields: fields_of(...) of a valid line of `layout`."""
    cols, width, _ = LAYOUTS[layout]
    pos = cols[1]
    if family == "empty_field":
        return _join(_with(fields, cols[2], "")), REASONS["empty_field"]
    if family == "too_few":
        return _join(fields[:max(cols)]), REASONS["too_few"]
    if family == "too_many":
        return _join(fields + ["x"]), REASONS["too_many"]
    if family in ("plus", "space", "underscore", "digits19"):
        value = {"plus": "+5", "space": " 5", "underscore": "1_000", "digits19": "1" * 19}[family]
        return _join(_with(fields, pos, value)), REASONS["bad_position"]
    if family == "blank":
        return b"", REASONS["empty_line"]
    raw = _join(fields)
    if family == "lone_cr":
        return raw[:1] + b"\r" + raw[1:], REASONS["lone_cr"]
    if family == "nul":
        return raw[:-1] + b"\0" + raw[-1:], REASONS["nul"]
    if family == "high":
        return b"\xc3\xa9" + raw, REASONS["high"]
    if family == "too_long":
        first = [k for k in range(width) if k not in cols][0]
        return _join(_with(fields, first, "r" * (MAX_LINE + 1 - len(raw) + len(fields[first])))), REASONS["too_long"]
    raise KeyError(family)


FAMILIES = ("empty_field", "too_few", "too_many", "plus", "space", "underscore", "digits19", "blank", "lone_cr", "nul", "high",
            "too_long")


# ---- the grammar, restated ---------------------------------------------------------------------------------------------------------
def model_line(raw, terminated, columns, width, ids):
    """One line: raw = its bytes without the '\\n', terminated = a '\\n' follows.  Returns (0, (c1, p1, c2, p2)) or (reason, None):
    the first defect from the left, field counts and empty fields being met where the field or the line ends."""
    need = max(columns) + 1
    role = {c: k for k, c in enumerate(columns)}
    field, start, out = 0, 0, [None] * 4
    n = len(raw)
    for i in range(n + 1):
        if i > MAX_LINE:
            return REASONS["too_long"], None
        line_ends = i == n
        field_ends = line_ends
        if not line_ends:
            b = raw[i]
            if b == 13:
                if i + 1 == n and terminated:
                    line_ends = field_ends = True
                else:
                    return REASONS["lone_cr"], None
            elif b == 9:
                field_ends = True
            elif b == 0:
                return REASONS["nul"], None
            elif b >= 0x80:
                return REASONS["high"], None
            elif role.get(field) in (1, 3) and (not 48 <= b <= 57 or i - start >= 18):
                return REASONS["bad_position"], None
        if not field_ends:
            continue
        if line_ends and i == 0:
            return REASONS["empty_line"], None
        if field in role:
            value = raw[start:i]
            if not value:
                return REASONS["empty_field"], None
            out[role[field]] = int(value) if role[field] in (1, 3) else ids.get(value, -1)
        field += 1
        if line_ends:
            return (REASONS["too_few"], None) if field < need else (0, tuple(out))
        if field >= width:
            return REASONS["too_many"], None
        start = i + 1
    raise AssertionError("unreachable")


def model_text(text, columns, width, names):
    """What cs_pairs_text_parse must report for `text`: (n_lines, first flagged line or -1, its reason or 0, the four columns or
    None when a line is flagged).  names: bytes, in genome order."""
    ids = {bytes(name): k for k, name in enumerate(names)}
    parts = bytes(text).split(b"\n")
    ended = parts[-1] == b""
    if ended:
        parts.pop()
    rows, flagged, reason = [], -1, 0
    for k, raw in enumerate(parts):
        verdict, row = model_line(raw, ended or k + 1 < len(parts), columns, width, ids)
        if verdict and flagged < 0:
            flagged, reason = k, verdict
        rows.append(row)
    if flagged >= 0:
        return len(parts), flagged, reason, None
    cols = tuple(np.asarray([r[k] for r in rows], dtype=dt) for k, dt in enumerate((np.int32, np.int64, np.int32, np.int64)))
    return len(parts), -1, 0, cols


# ---- the record file of tools/pairs_text_check.cpp -----------------------------------------------------------------------------------
def write_record_file(path, records):
    """records: (columns, width, names as bytes, text) -- the expectation is model_text's."""
    with open(path, "wb") as f:
        f.write(b"CSPT" + struct.pack("<I", len(records)))
        for columns, width, names, text in records:
            n_lines, flagged, reason, cols = model_text(text, columns, width, names)
            f.write(struct.pack("<5iI", *columns, width, len(names)))
            for name in names:
                f.write(struct.pack("<I", len(name)) + name)
            f.write(struct.pack("<I", len(text)) + text)
            f.write(struct.pack("<qqi", n_lines, flagged, reason))
            if flagged < 0:
                for col, dt in zip(cols, ("<i4", "<i8", "<i4", "<i8")):
                    f.write(np.ascontiguousarray(col, dtype=dt).tobytes())


def corrupted(rng, text):
    """One seeded corruption of a text: a byte replaced, inserted or removed, a stretch cut out or doubled."""
    data = bytearray(text)
    special = b"\t\n\r\0\x80\xff +-_09a"
    kind = int(rng.integers(5))
    at = int(rng.integers(len(data))) if data else 0
    pick = special[int(rng.integers(len(special)))] if rng.random() < 0.7 else int(rng.integers(256))
    if kind == 0 and data:
        data[at] = pick
    elif kind == 1:
        data.insert(at, pick)
    elif kind == 2 and data:
        del data[at]
    elif kind == 3 and data:
        del data[at:at + int(rng.integers(1, 40))]
    elif data:
        data[at:at] = data[at:at + int(rng.integers(1, 40))]
    return bytes(data)
