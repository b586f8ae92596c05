"""The host side of the device .cool decode: hdf5_lite.File.chunk_index against the per-entry walk of File.dataset, the rule by which
open_cool(decode="auto") picks its route, and the decoder core of cs_inflate.hip (cs_inflate_core.h) as a host program under the
address and undefined-behaviour sanitizers (tools/inflate_check.cpp) on valid and corrupted streams.  No GPU."""
import pathlib
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from chromosight_amd import hdf5_lite, pipeline
from tests import inflate_util as iu

ROOT = pathlib.Path(__file__).resolve().parents[1]
EXAMPLE = ROOT / "tests" / "golden" / "example.cool"
CSRC = ROOT / "chromosight_amd" / "csrc"


# ---- chunk_index ------------------------------------------------------------------------------------------------------------------
def _walk_per_entry(f, path):
    """The chunks of a dataset in the order File.dataset visits them, read as it reads them: one struct.unpack_from per entry."""
    layout = [d for t, d in f.messages(f.resolve(path)) if t == 0x08][0]
    if layout[1] != 2:
        return None
    rank = layout[2]
    btree, = struct.unpack_from("<Q", layout, 3)
    out = []

    def walk(node):
        p = f.base + node
        level, n_ent = f.buf[p + 5], struct.unpack_from("<H", f.buf, p + 6)[0]
        q = p + 24
        key = 8 + 8 * rank
        for _ in range(n_ent):
            nbytes, mask = struct.unpack_from("<II", f.buf, q)
            start, = struct.unpack_from("<Q", f.buf, q + 8)
            child, = struct.unpack_from("<Q", f.buf, q + key)
            if level:
                walk(child)
            else:
                out.append((f.base + child, nbytes, start, mask))
            q += key + 8
    if btree != hdf5_lite.UNDEF:
        walk(btree)
    return out


def _all_datasets(f, addr=None, prefix=""):
    addr = f.root if addr is None else addr
    for name, child in f.links(addr).items():
        types = {t for t, _ in f.messages(child)}
        if 0x11 in types:
            yield from _all_datasets(f, child, f"{prefix}/{name}")
        elif 0x08 in types:
            yield f"{prefix}/{name}"


def test_chunk_index_matches_the_per_entry_walk_and_decodes_to_dataset():
    chunked = 0
    with hdf5_lite.File(EXAMPLE) as f:
        for path in _all_datasets(f):
            want = _walk_per_entry(f, path)
            if want is None:
                with pytest.raises(hdf5_lite.Hdf5Unsupported):
                    f.chunk_index(path)
                continue
            chunked += 1
            idx = f.chunk_index(path)
            got = list(zip(idx.offsets.tolist(), idx.nbytes.tolist(), idx.starts.tolist(), idx.masks.tolist()))
            assert got == want, path
            column = f.dataset(path)
            assert idx.dtype == column.dtype and idx.length == column.size
            out = np.zeros(idx.length, dtype=idx.dtype)
            for off, nb, start, mask in got:
                raw = bytes(f.buf[off:off + nb])
                for k, (fid, _) in reversed(list(enumerate(idx.filters))):
                    if mask & (1 << k):
                        continue
                    if fid == 1:
                        raw = zlib.decompress(raw)
                    elif fid == 2:
                        raw = iu.unshuffle(raw, idx.dtype).tobytes()
                    else:
                        raise AssertionError(f"{path}: filter {fid}")
                vals = np.frombuffer(raw, dtype=idx.dtype, count=idx.chunk)
                m = min(idx.chunk, idx.length - start)
                out[start:start + m] = vals[:m]
            assert out.tobytes() == column.tobytes(), path
    assert chunked >= 3                                   # the three pixel columns at the least


# ---- the qualifying rule ----------------------------------------------------------------------------------------------------------
def _index(dtype="<i8", length=5000, chunk=1899, filters=((2, (8,)), (1, (6,)))):
    n = -(-length // chunk)
    return hdf5_lite.ChunkIndex(np.dtype(dtype), length, chunk, tuple(filters), np.arange(n, dtype=np.int64) * 100, np.full(n, 100, dtype=np.int64),
                                np.arange(n, dtype=np.int64) * chunk, np.zeros(n, dtype=np.uint32))


LIMIT = 128 * 1024


def test_integer_chunked_columns_within_the_limit_qualify():
    assert pipeline.device_decode_refusal({"bin1_id": _index(), "bin2_id": _index(), "count": _index("<i4")}, LIMIT) is None
    fl = _index(filters=((2, (8,)), (1, (6,)), (3, ())))
    assert pipeline.device_decode_refusal({"bin1_id": fl, "bin2_id": fl, "count": fl}, LIMIT) is None
    plain = _index(filters=())
    assert pipeline.device_decode_refusal({"bin1_id": plain, "bin2_id": plain, "count": plain}, LIMIT) is None


@pytest.mark.parametrize("what, bad", [
    ("float counts", lambda: _index("<f8")),
    ("contiguous layout", lambda: None),
    ("an unknown filter id", lambda: _index(filters=((2, (8,)), (32015, ())))),
    ("an oversized chunk", lambda: _index(chunk=LIMIT // 8 + 1, length=100_000)),
    ("filters in another order", lambda: _index(filters=((1, (6,)), (2, (8,))))),
    ("unsigned counts", lambda: _index("<u4")),
])
def test_what_does_not_qualify_goes_to_the_host_route(what, bad):
    reason = pipeline.device_decode_refusal({"bin1_id": _index(), "bin2_id": _index(), "count": bad()}, LIMIT)
    assert isinstance(reason, str) and "count" in reason, what


def test_decode_argument_is_checked_and_the_environment_forces_the_host(monkeypatch):
    with pytest.raises(ValueError, match="decode"):
        pipeline.open_cool(str(EXAMPLE), decode="gpu")
    with pytest.raises(ValueError, match="dictionary"):
        pipeline.open_cool({"binsize": 1}, decode="device")
    monkeypatch.setenv("CHROMOSIGHT_HIP_HOST_DECODE", "1")
    assert pipeline._decode_route("auto") == "host"
    with pytest.raises(ValueError, match="CHROMOSIGHT_HIP_HOST_DECODE"):
        pipeline._decode_route("device")
    monkeypatch.delenv("CHROMOSIGHT_HIP_HOST_DECODE")
    assert pipeline._decode_route("auto") == "auto" and pipeline._decode_route("host") == "host"
    monkeypatch.setenv("CHROMOSIGHT_H5DUMP_ONLY", "1")                 # the file is then not read natively: nothing for the device
    with pytest.raises(pipeline.DeviceDecodeRefused, match="CHROMOSIGHT_H5DUMP_ONLY"):
        pipeline.DeviceCool.from_cool_file(str(EXAMPLE))


# ---- the decoder core under the sanitizers ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker():
    if shutil.which("g++") is None or shutil.which("make") is None:
        pytest.skip("no host C++ compiler")
    subprocess.run(["make", "-C", str(CSRC), "inflate_check"], check=True, capture_output=True)
    return CSRC / "build" / "inflate_check"


def _run(checker, tmp_path, records):
    path = tmp_path / "streams.bin"
    iu.write_stream_file(path, records)
    res = subprocess.run([str(checker), str(path)], capture_output=True, text=True)
    assert res.returncode == 0, f"inflate_check ended with {res.returncode} (a sanitizer report?)\n{res.stderr[-4000:]}"
    lines = [tuple(int(x) for x in line.split()) for line in res.stdout.splitlines()]
    assert len(lines) == len(records)
    return lines


def test_the_stream_list_is_what_zlib_says():
    iu.check_cases_against_zlib()


def test_core_decodes_the_stream_list(checker, tmp_path):
    streams = iu.gzip_streams()
    got = _run(checker, tmp_path, [(s, len(raw), raw) for _, s, raw in streams])
    for (name, _, _), (status, equal) in zip(streams, got):
        assert (status, equal) == (0, 1), name


def test_core_names_every_failure(checker, tmp_path):
    cases = iu.failure_streams()
    assert {s for s, *_ in cases} == set(range(1, 10))
    got = _run(checker, tmp_path, [(stream, cap, None) for _, _, stream, cap in cases])
    for (want, label, stream, _), (status, _) in zip(cases, got):
        assert status == want, label
        if want not in (6, 7):                            # too long / too short are about the chunk, not about the stream
            assert iu.zlib_verdict(stream) is None, label


def test_core_survives_corrupted_streams(checker, tmp_path):
    """Each of 2 400 corruptions ends in an error status or in the bytes zlib itself gives, never in a sanitizer report (which
    would end the program with a non-zero status)."""
    cases = list(iu.corruptions(2400))
    verdicts = [iu.zlib_verdict(stream) for _, stream, _ in cases]
    got = _run(checker, tmp_path, [(stream, cap, v) for (_, stream, cap), v in zip(cases, verdicts)])
    n_err = 0
    for (label, _, cap), verdict, (status, equal) in zip(cases, verdicts, got):
        assert status != 0 or equal == 1, label
        if verdict is not None and len(verdict) == cap:
            assert (status, equal) == (0, 1), label        # what zlib takes at the chunk's size, the decoder takes too
        n_err += status != 0
    assert n_err > 1000                                   # (the corruptions do corrupt)
