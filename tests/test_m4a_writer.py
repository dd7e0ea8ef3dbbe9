"""mp4.write_m4a, the container writer behind save(), on the CPU: what it writes is read back by the package's demuxer
(mp4.find_alac_track), by the C++ demuxer (host/mp4_demux.hpp through the shim tests/test_container.py builds) and by a
plain box walk of this file's own."""
import importlib
import struct

import numpy as np
import pytest

from tests import test_container as tc

VARIANTS = [{}, {"_co64": True}, {"_large_mdat": True}, {"_co64": True, "_large_mdat": True}]


@pytest.fixture(scope="module")
def mp4(pkg):
    return importlib.import_module("saprobe-alac_amd.mp4")


def cookie_of(fl=4096, depth=16, ch=2, rate=44100, max_frame=1234, bit_rate=567890):
    return struct.pack(">IBBBBBBHIII", fl, 0, depth, 40, 10, 14, ch, 255, max_frame, bit_rate, rate)


def some_packets(rng, n):
    sizes = rng.integers(1, 400, n)
    offsets = np.zeros(n + 1, np.uint64)
    offsets[1:] = np.cumsum(sizes)
    return rng.integers(0, 256, int(offsets[-1]), dtype=np.uint8), offsets


def boxes(data, start=0, end=None, path=b""):
    """Every box of the file as (path, payload) in file order, containers walked into."""
    end = len(data) if end is None else end
    pos = start
    while pos < end:
        size, cc = struct.unpack(">I4s", data[pos:pos + 8])
        header = 8
        if size == 1:
            size, header = struct.unpack(">Q", data[pos + 8:pos + 16])[0], 16
        assert header <= size <= end - pos, (cc, size)
        yield path + b"/" + cc, data[pos + header:pos + size]
        if cc in (b"moov", b"trak", b"mdia", b"minf", b"stbl", b"dinf"):
            yield from boxes(data, pos + header, pos + size, path + b"/" + cc)
        pos += size


@pytest.mark.parametrize("kw", VARIANTS)
@pytest.mark.parametrize("last", [4096, 1, 1000])
def test_written_file_parses_back(pkg, mp4, kw, last):
    rng = np.random.default_rng(last)
    n = 23
    blob, offsets = some_packets(rng, n)
    total = (n - 1) * 4096 + last
    cookie = cookie_of()
    data = mp4.write_m4a(cookie, blob, offsets, total, 44100, 2, 16, **kw)
    t = mp4.find_alac_track(data)
    # the sample entry's child is the 36-byte 'alac' full box around the cookie: ParseMagicCookie skips its header
    assert bytes(t.cookie) == struct.pack(">I4sI", 36, b"alac", 0) + cookie
    cfg, want = pkg.ParseMagicCookie(t.cookie), pkg.ParseMagicCookie(cookie)
    assert bytes(cfg) == bytes(want) and cfg.FrameLength == 4096 and cfg.MaxFrameBytes == 1234 and cfg.AvgBitRate == 567890
    sizes = np.diff(offsets.astype(np.int64))
    assert np.array_equal(t.sizes, sizes) and t.contiguous()
    for i in (0, 1, n // 2, n - 1):
        o = int(t.offsets[i])
        assert data[o:o + int(sizes[i])] == blob[int(offsets[i]):int(offsets[i + 1])].tobytes()
    assert int(t.offsets[-1]) + int(sizes[-1]) == len(data)  # mdat is the file's last box and ends with the last packet

    tree = list(boxes(data))
    names = [p for p, _ in tree]
    assert [p for p in names if p.count(b"/") == 1] == [b"/ftyp", b"/moov", b"/mdat"]
    assert names.count(b"/moov/trak") == 1
    for must in (b"/moov/mvhd", b"/moov/trak/tkhd", b"/moov/trak/mdia/mdhd", b"/moov/trak/mdia/hdlr", b"/moov/trak/mdia/minf/smhd",
                 b"/moov/trak/mdia/minf/dinf/dref", b"/moov/trak/mdia/minf/stbl/stsd", b"/moov/trak/mdia/minf/stbl/stts",
                 b"/moov/trak/mdia/minf/stbl/stsc", b"/moov/trak/mdia/minf/stbl/stsz"):
        assert names.count(must) == 1, must
    stbl = b"/moov/trak/mdia/minf/stbl/"
    assert (stbl + b"co64" in names) == bool(kw.get("_co64")) and (stbl + b"stco" in names) != bool(kw.get("_co64"))
    mdat_at = data.rfind(b"mdat", 0, int(t.offsets[0]))
    assert (struct.unpack(">I", data[mdat_at - 4:mdat_at])[0] == 1) == bool(kw.get("_large_mdat"))
    get = dict(tree)
    mdhd = get[b"/moov/trak/mdia/mdhd"]
    assert struct.unpack(">II", mdhd[12:20]) == (44100, total)  # timescale = sample rate, duration = frames
    assert get[b"/moov/trak/mdia/hdlr"][8:12] == b"soun"
    assert struct.unpack(">I", get[b"/moov/trak/tkhd"][20:24])[0] == total
    stts = get[stbl + b"stts"]
    runs = [struct.unpack(">II", stts[8 + 8 * k:16 + 8 * k]) for k in range(struct.unpack(">I", stts[4:8])[0])]
    assert sum(c * d for c, d in runs) == total and sum(c for c, _ in runs) == n
    assert runs == ([(n, 4096)] if last == 4096 else [(n - 1, 4096), (1, last)])
    assert struct.unpack(">IIII", get[stbl + b"stsc"][4:20]) == (1, 1, n, 1)  # one chunk with every sample
    stsd = get[stbl + b"stsd"]
    assert stsd[12:16] == b"alac" and struct.unpack(">HH", stsd[32:36]) == (2, 16) and struct.unpack(">I", stsd[40:44])[0] == 44100 << 16


@pytest.mark.parametrize("kw", VARIANTS)
def test_cpp_demuxer_reads_the_written_file(mp4, kw):
    L = tc._build_shim(False)
    rng = np.random.default_rng(9)
    for n, last, depth, ch in ((1, 7, 24, 2), (40, 4096, 16, 2), (17, 33, 32, 8)):
        blob, offsets = some_packets(rng, n)
        data = mp4.write_m4a(cookie_of(depth=depth, ch=ch), blob, offsets, (n - 1) * 4096 + last, 48000, ch, depth, **kw)
        got = tc._cpp_demux(L, data)
        assert not isinstance(got, str), got
        t = mp4.find_alac_track(data)
        assert got[0] == bytes(t.cookie) and np.array_equal(got[1], t.offsets) and np.array_equal(got[2], t.sizes)
        assert np.array_equal(got[2], np.diff(offsets.astype(np.int64)))


@pytest.mark.parametrize("kw", VARIANTS)
def test_no_packets_is_a_file_with_an_empty_track(pkg, mp4, kw):
    cookie = cookie_of()
    data = mp4.write_m4a(cookie, b"", np.zeros(1, np.uint64), 0, 44100, 2, 16, **kw)
    t = mp4.find_alac_track(data)
    assert len(t) == 0 and bytes(t.cookie)[12:] == cookie
    got = tc._cpp_demux(tc._build_shim(False), data)
    assert not isinstance(got, str) and len(got[1]) == 0 and got[0] == bytes(t.cookie)
    get = dict(boxes(data))
    assert struct.unpack(">I", get[b"/moov/trak/mdia/minf/stbl/stts"][4:8])[0] == 0
    assert get[b"/mdat"] == b""


def test_a_window_of_the_blob_and_bad_arguments(mp4):
    """offsets need not start at 0 (the packets of a larger blob); what cannot be a file raises."""
    rng = np.random.default_rng(2)
    blob, offsets = some_packets(rng, 10)
    data = mp4.write_m4a(cookie_of(fl=100), blob, offsets[4:], 6 * 100, 44100, 2, 16)
    t = mp4.find_alac_track(data)
    assert data[int(t.offsets[0]):] == blob[int(offsets[4]):].tobytes()
    for bad in (lambda: mp4.write_m4a(cookie_of()[:20], blob, offsets, 10 * 4096, 44100, 2, 16),
                lambda: mp4.write_m4a(cookie_of(), blob, offsets, 10 * 4096 + 1, 44100, 2, 16),
                lambda: mp4.write_m4a(cookie_of(), blob, offsets, 9 * 4096, 44100, 2, 16),
                lambda: mp4.write_m4a(cookie_of(), blob[:-1], offsets, 10 * 4096, 44100, 2, 16),
                lambda: mp4.write_m4a(cookie_of(), blob, offsets[::-1], 10 * 4096, 44100, 2, 16)):
        with pytest.raises(ValueError):
            bad()
