"""``hisat2.packAlignments(decode="device")`` where the device route does not apply -- SAM text, or a ``.bam`` whose text
is kept: the host route's result, one warning per process; and its argument errors.  No GPU is touched."""
import logging

import pytest

from ingest_cases import headerOf, smallIndex
from kir_graph_amd import hisat2, packed, synth
from kir_graph_amd.utils import logger


def comparable(pack):
    text = pack["pairs_text"]
    return (pack["records"].tobytes(), list(pack["strings"]), dict(pack["counts"]),
            None if text is None else (text.blob, text.pair_lines.tolist()))


def test_device_decode_takes_the_host_route_for_other_inputs(tmp_path, monkeypatch):
    sidx, gidx = smallIndex()
    lines = synth.toSamLines(synth.makeSample(sidx, seed=21, n_pairs=300))
    chunks = [("\n".join(lines) + "\n").encode()]
    bam = str(tmp_path / "s.bam")
    packed.writeBam(bam, "\n".join(headerOf(sidx, "unsorted") + lines) + "\n")
    monkeypatch.setattr(hisat2, "_decode_warned", False)
    seen = []
    handler = logging.Handler()
    handler.emit = lambda record: seen.append((record.levelno, record.getMessage()))
    logger.addHandler(handler)
    try:
        for source, keep_text in ((chunks, True), (chunks, False), (bam, True)):
            want = hisat2.packAlignments(source, gidx, keep_text=keep_text)
            got = hisat2.packAlignments(source, gidx, keep_text=keep_text, decode="device")      # no context needed
            assert "mates" not in got and "decode" not in got["counts"]
            assert comparable(got) == comparable(want) and want["counts"]["pairs"] == 300
    finally:
        logger.removeHandler(handler)
    warnings = [m for level, m in seen if level == logging.WARNING and "ingest decode" in m]
    assert len(warnings) == 1 and "decoded on the host" in warnings[0], seen
    assert hisat2._decode_warned is True


def test_device_decode_argument_errors(tmp_path):
    sidx, gidx = smallIndex()
    lines = synth.toSamLines(synth.makeSample(sidx, seed=21, n_pairs=20))
    bam = str(tmp_path / "s.bam")
    packed.writeBam(bam, "\n".join(headerOf(sidx, "unsorted") + lines) + "\n")
    with pytest.raises(ValueError, match="needs a device context"):
        hisat2.packAlignments(bam, gidx, keep_text=False, decode="device")
    with pytest.raises(ValueError, match="'host' or 'device'"):
        hisat2.packAlignments(bam, gidx, keep_text=False, decode="gpu")
