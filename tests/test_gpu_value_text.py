"""The value-text emitter on the GPU (decimal6.h g6_text, model_codec.hip k_vtext_*):
`ostream << float` for runs of values, formatted on the device, against libc's '%g'
(the exhaustive digest of tests/native/check_g6text.cpp) and Python's '%g'."""
import json
import os

import numpy as np
import pytest

import g6_edges

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _lines(vals, sizes):
    out, o = [], 0
    for s in sizes:
        out.append("".join(g6_edges.g_text(int(b)) + " " for b in vals[o:o + s].view(np.uint32)) + "\n")
        o += s
    return "".join(out).encode()


def _pairs(vals):
    return "".join(f"{i}\n{g6_edges.g_text(int(b))}\n" for i, b in enumerate(vals.view(np.uint32))).encode()


def _run(n):
    """n values: the edge list, repeated"""
    e = g6_edges.edge_values()
    return np.resize(e, n).copy()


def test_text_digest_over_every_binary32(codec):
    """fn 24: the text of all 2^32 bit patterns, digested on the GPU, equals the digest of
    libc's snprintf("%g") (and the six fixed strings for inf / nan)."""
    ref = json.load(open(os.path.join(HERE, "golden", "g6text_digest.json")))
    assert f"{codec.selftest_digest(24):016x}" == ref["fn24"]


@pytest.mark.parametrize("sizes", [
    [255, 256, 257],            # value runs ending at 255, 256 and 257 values: around one launch block
    [256, 0, 257],              # a block of size 0 between two others
    [1, 1, 0, 0, 1, 300, 0],    # one-value blocks, empty blocks in a row and at the end
    [0, 0, 61],                 # empty blocks before the first value
    [0],                        # nothing but an empty block
])
def test_lines_match_python(codec, sizes):
    v = _run(sum(sizes))
    assert codec.values_text(v, sizes) == _lines(v, sizes)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1001])
def test_dictionary_pairs_match_python(codec, n):
    v = _run(n)
    assert codec.values_text(v) == _pairs(v)


def test_device_values_are_read_in_place(codec):
    import torch
    sizes = [61, 0, 257]
    v = _run(sum(sizes))
    d = torch.from_numpy(v.view(np.int32)).cuda().view(torch.float32)  # bits kept: NaN payloads travel as ints
    assert codec.values_text(d, sizes) == _lines(v, sizes)
    assert codec.values_text(d) == _pairs(v)


def test_bad_blocks_are_refused(codec):
    import fleet_amd
    v = _run(10)
    with pytest.raises(fleet_amd.FleetError):
        codec.values_text(v, [4, 5])          # the blocks do not hold the values
    with pytest.raises(fleet_amd.FleetError):
        codec.values_text(v, [11, -1])
    with pytest.raises(fleet_amd.FleetError):
        codec.values_text(v, [5] + [0] * 255 + [5])   # more empty blocks in a row than a cell counts
    for sizes in ([5] + [0] * 254 + [5], [0] * 254 + [10], [10] + [0] * 254):
        assert codec.values_text(v, sizes) == _lines(v, sizes)
