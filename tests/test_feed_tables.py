"""CPU side of the precode parity on synthetic tables (tests/feed_tables.py,
tests/test_gpu_feed_tables.py): the generator's coverage,
computed from the tables, the planes and the oracle's per-list counts, and the
host precode and payload (entropy.cpp) against the oracle's walk
(orc_precode_slice / orc_serialize_slice) on every case, the frames over the
feed capacity included.  Everything is exact: bit counts, words and bytes."""
import functools

import numpy as np
import pytest

from tests import feed_tables as ft

CAP = ft.CAPACITY


@functools.lru_cache(maxsize=None)
def reference():
    """Every case with the oracle's feed, computed once per process and shared
    with the GPU tests: name -> dict(wmb, hmb, ring, table, planes, words, bits,
    lists, dropped)."""
    from oracle import oracle

    out = {}
    for name, wmb, hmb, ring, table, planes in ft.cases():
        words, bits, lists, dropped = oracle.precode_slice(table, wmb, hmb, ring, *planes)
        for a in (table, words, *planes):
            a.setflags(write=False)
        out[name] = dict(wmb=wmb, hmb=hmb, ring=ring, table=table, planes=planes, words=words, bits=bits, lists=lists,
                         dropped=dropped)
    return out


@pytest.fixture(scope="module")
def ref(orc):
    return reference()


# ---------------------------------------------------------------------------
# What a case holds, from its table and planes
# ---------------------------------------------------------------------------

def _present(c, field):
    """Macroblock indices of a delta list's items, their values and coded deltas."""
    return ft.delta_items(c["table"], field)


def _chunks_with(idx):
    return set((idx // ft.CHUNK).tolist())


def _gap(members):
    """Does the sorted set hold a, b with b > a + 1 and nothing between?"""
    s = sorted(members)
    return any(b > a + 1 for a, b in zip(s, s[1:]))


def _coded(c):
    """(coded values (n, 6, 64) of the non-copy macroblocks in coding order, their indices)."""
    keep = np.flatnonzero((c["table"]["block_type"] & ft.COPY) == 0)
    return ft.coded_blocks(c["planes"], c["wmb"], c["hmb"])[keep], keep


def _attempted(c):
    """Bits the Y, U and V sections try to write (plain restatement of the code lengths)."""
    coded, _ = _coded(c)
    bits = ft.block_bits(coded)
    return int(bits[:, :4].sum()), int(bits[:, 4].sum()), int(bits[:, 5].sum())


DELTA_FIELDS = ("motion_x", "motion_y", "q_index")


def test_generator_coverage(ref):
    """Every class the cases are aimed at really occurs.  A gap in the
    generator fails here, not silently on the GPU."""
    assert tuple(ref) == ft.NAMES
    for name, c in ref.items():
        ft.assert_value_range(c["table"], c["planes"], c["wmb"], c["hmb"])  # the excluded value
        assert c["bits"] == sum(c["lists"])
        if name not in ft.OVER_CAPACITY:
            assert c["dropped"] == 0 and tuple(c["lists"][8:]) == _attempted(c), name

    for f in DELTA_FIELDS:
        found = set()
        for name, c in ref.items():
            idx, val, delta = _present(c, f)
            mbs = c["wmb"] * c["hmb"]
            if not idx.size:
                found.add("empty list")
                continue
            chunks = _chunks_with(idx)
            if _gap(chunks):
                found.add("empty chunks between chunks with items")
            if min(chunks) > 0:
                found.add("first item past chunk 0")
            if max(chunks) > ft.TILE and min(chunks) < ft.TILE - 1 and (ft.TILE - 1 in chunks or ft.TILE in chunks):
                found.add("items on both sides of the carry tile's edge")
            for ch in chunks:
                inside = idx[idx // ft.CHUNK == ch]
                waves = (inside % ft.CHUNK) // ft.WAVE
                if _gap(set(waves.tolist())):
                    found.add("empty waves between waves with items")
                for w in set(waves.tolist()):
                    lanes = inside[waves == w] % ft.WAVE
                    if lanes.size == 1:
                        found.add(f"alone in its wave on lane {int(lanes[0])}")
            plain = np.diff(val, prepend=0)
            if (plain != delta).any():
                found.add("delta wraps")
            if f != "q_index":
                if (ft.se_len(delta) == 31).any():
                    found.add("31-bit code")
                if {-32768, 32767} <= set(val.tolist()) and any(a == 32767 and b == -32768 for a, b in zip(val, val[1:])):
                    found.add("32767 then -32768")
            elif set(val.tolist()) == {1, 31} and (np.abs(delta[1:]) == 30).all() and mbs >= ft.CHUNK:
                found.add("alternating 1 and 31")
        want = {"empty list", "empty chunks between chunks with items", "first item past chunk 0",
                "items on both sides of the carry tile's edge", "empty waves between waves with items",
                "alone in its wave on lane 0", "alone in its wave on lane 63"}
        want |= {"alternating 1 and 31"} if f == "q_index" else {"delta wraps", "31-bit code", "32767 then -32768"}
        assert not want - found, (f, sorted(want - found))

    # geometry: macroblock counts with partial waves, workgroups and chunks; every ring size
    assert {1, 3, 255, 256, 257, 1023, 16641} <= {c["wmb"] * c["hmb"] for c in ref.values()}
    assert {c["ring"] for c in ref.values()} == set(range(1, ft.MAX_RING + 1))
    for ring in range(1, ft.MAX_RING + 1):
        mask = (1 << (ring.bit_length() - 1)) - 1
        assert any(c["ring"] == ring and (c["table"]["prediction_target"].astype(int) > mask)[(c["table"]["block_type"] & 1) == 0]
                   .any() for c in ref.values()), ring

    # descriptor values
    t = np.concatenate([c["table"] for c in ref.values()])
    motion = (t["block_type"] & ft.MOTION) != 0
    assert (motion & (t["sp_pred"] == 2)).any() and (motion & (t["sp_pred"] > 2) & (t["sp_pred"] & 1 == 0)).any()
    assert (motion & (t["sp_pred"] != 0) & (t["sp_amount"] > 1)).any()
    assert (motion & (t["sp_pred"] != 0) & (t["sp_index"] > 7)).any()
    assert ((t["block_type"] & 7) == 5).any() and (t["block_type"] > 7).any() and (t["block_type"] >= 1 << 31).any()

    # coefficient blocks and the start bit of every block modulo 32
    found, residues, per_case = set(), set(), {}
    for name, c in ref.items():
        coded, keep = _coded(c)
        if not keep.size:
            continue
        here = per_case[name] = set()
        bits = ft.block_bits(coded)
        order = np.concatenate([bits[:, :4].ravel(), bits[:, 4], bits[:, 5]])  # the blocks in feed order
        if name not in ft.OVER_CAPACITY:
            starts = sum(c["lists"][:8]) + np.cumsum(order) - order
            residues |= set((starts % 32).tolist())
        luma = bits[:, :4].ravel()
        if ((luma[:-1] == ft.FULL_BLOCK) & (luma[1:] == 1)).any() and ((luma[:-1] == 1) & (luma[1:] == ft.FULL_BLOCK)).any():
            here.add("full block beside an all-zero block")
        nz = coded != 0
        if (nz.sum(-1) == 1)[nz[..., 0]].any():
            here.add("run 1")
        if (nz[..., 63] & (nz.sum(-1) == 1)).any():
            here.add("only position 63")
        if (coded == 32767).any() and (coded == -32767).any():
            here.add("+-32767")
        for k in (0, 4, 5):
            if (ft.se_len(coded[..., k, :]) == 31).any():
                here.add(f"31-bit code in {'YUV'[k and k - 3]}")
        # the DC chain
        wmb = c["wmb"]
        raw = ft._blocks_of(c["planes"], wmb, c["hmb"]).astype(np.int64)
        copy = (c["table"]["block_type"] & ft.COPY) != 0
        mx, my = keep % wmb, keep // wmb
        above = keep[(mx == 0) & (my > 0)] - wmb
        if (~copy[above] & (raw[above, 2, 0] != 0) & (raw[above, 4, 0] != 0)).any():
            here.add("first column takes the block above")
        if (copy[above] & (raw[above, 2, 0] != 0) & (raw[above, 4, 0] != 0)).any():
            here.add("first column takes a copy macroblock's stale values")
        left = keep[mx > 0] - 1
        if (copy[left] & (raw[left, 1, 0] != 0) & (raw[left, 4, 0] != 0)).any():
            here.add("stale values of a copy macroblock on the left")
        dc = raw[keep][:, :, 0]
        if (np.abs(dc[:, 1] - dc[:, 0]) > 32767).any() and (np.abs(dc[:, 3] - dc[:, 2]) > 32767).any():
            here.add("delta wraps inside a macroblock")
        if (np.abs(dc[mx > 0][:, 4] - raw[left, 4, 0]) > 32767).any():
            here.add("chroma delta wraps")
        if (dc[:, 0] != 0).any() and (dc[:, 2] != 0).any() and (coded[:, 1:4, 0] != raw[keep][:, 1:4, 0]).any():
            here.add("TL -> TR / BL -> BR chain")
        found |= here
    dc_classes = {"first column takes the block above", "first column takes a copy macroblock's stale values",
                  "stale values of a copy macroblock on the left", "delta wraps inside a macroblock",
                  "chroma delta wraps", "TL -> TR / BL -> BR chain"}
    blocks = {"full block beside an all-zero block", "run 1", "only position 63", "+-32767", "31-bit code in Y",
              "31-bit code in U", "31-bit code in V"}
    # the two directed cases hold their classes themselves, not only the set as a whole
    assert not dc_classes - per_case["dc_chain"], sorted(dc_classes - per_case["dc_chain"])
    assert not blocks - per_case["extreme_blocks"], sorted(blocks - per_case["extreme_blocks"])
    want = dc_classes | blocks
    assert not want - found, sorted(want - found)
    assert residues == set(range(32)), sorted(set(range(32)) - residues)

    # capacity: totals from the oracle's counts
    at, one, fits, uo = (ref[n] for n in ("y_at_capacity", "y_one_bit_over", "y_over_with_fits", "u_over"))
    assert at["lists"][8] == CAP and at["dropped"] == 0 and _attempted(at)[0] == CAP
    assert _attempted(one)[0] == CAP + 1 and one["dropped"] == 1 and CAP - 30 <= one["lists"][8] <= CAP
    y_try = _attempted(fits)[0]
    # the first write dropped (31 bits, 10 bits before the end) is followed by writes that fit: the section fills up
    assert y_try > CAP + 2000 and fits["dropped"] > 100 and fits["lists"][8] == CAP
    coded, _ = _coded(fits)
    cum = np.cumsum(ft.block_bits(coded)[:, :4].ravel())
    k = int(np.searchsorted(cum, CAP - 17, side="right"))   # the block that crosses the end
    assert cum[k - 1] == CAP - 17 and list(coded[k // 4, k % 4, :8]) == [20000, 1, -1, 1, -20000, 0, 1, -1]
    y_u, u_u, v_u = _attempted(uo)
    assert y_u <= CAP and v_u <= CAP and u_u > CAP and uo["lists"][9] <= CAP and uo["dropped"] > 0
    for c in (one, fits, uo):
        assert max(c["lists"][8:]) <= CAP


# ---------------------------------------------------------------------------
# The host precode and payload against the oracle's walk
# ---------------------------------------------------------------------------

def _host_equals_oracle(orc, cairo, c, name):
    words, bits = cairo.precode_slice(c["table"], c["wmb"], c["hmb"], c["ring"], *c["planes"])
    assert bits == c["bits"], (name, bits, c["bits"])
    np.testing.assert_array_equal(words, c["words"], err_msg=name)
    want = orc.serialize_slice(c["table"], c["wmb"], c["hmb"], c["ring"], *c["planes"])
    got = cairo.serialize_slice(c["table"], c["wmb"], c["hmb"], c["ring"], *c["planes"],
                                capacity_bytes=c["bits"] // 4 + 65536)
    assert got[1] == want[1], (name, got[1], want[1])
    assert got[0] == want[0], name


def test_host_matches_oracle(orc, cairo, ref):
    """cairo.precode_slice == oracle.precode_slice (words and bit count) and
    cairo.serialize_slice == oracle.serialize_slice on every case below the
    feed capacity."""
    for name, c in ref.items():
        if name not in ft.OVER_CAPACITY and name != "y_at_capacity":
            _host_equals_oracle(orc, cairo, c, name)


@pytest.mark.parametrize("name", ("y_at_capacity",) + ft.OVER_CAPACITY)
def test_host_drop_rule_matches_oracle(orc, cairo, ref, name):
    """The same at and over the capacity: the host's drop rule (a write that
    would pass 32 Mbit of a section is dropped whole, later ones that fit are
    kept) against the oracle's, the first such check off natural data."""
    _host_equals_oracle(orc, cairo, ref[name], name)


def test_minus_32768_rule(orc, cairo):
    """a coded value of -32768 (coefficient, DC delta, motion
    delta) is coded as -32767.  The host and the oracle on such a frame give
    the feed and payload of the frame that holds -32767 in those places, which
    uses no special rule."""
    for name, wmb, hmb, ring, table, planes in ft.rule_cases():
        coded = ft.coded_blocks(planes, wmb, hmb)[(table["block_type"] & ft.COPY) == 0]
        assert (coded[:, :, 0] == -32768).sum() >= 3 and (coded[:, :, 1:] == -32768).sum() >= 3
        for f in ("motion_x", "motion_y"):
            assert (ft.delta_items(table, f)[2] == -32768).any()
        t2, p2 = ft.rule_applied(table, planes, wmb, hmb)
        ft.assert_value_range(t2, p2, wmb, hmb)
        same = ft.coded_blocks(p2, wmb, hmb)[(table["block_type"] & ft.COPY) == 0]
        assert ((same == coded) | ((coded == -32768) & (same == -32767))).all()
        want = orc.precode_slice(t2, wmb, hmb, ring, *p2)
        assert want[3] == 0
        for got in (orc.precode_slice(table, wmb, hmb, ring, *planes)[:2], cairo.precode_slice(table, wmb, hmb, ring, *planes)):
            assert got[1] == want[1]
            np.testing.assert_array_equal(got[0], want[0])
        pay = orc.serialize_slice(t2, wmb, hmb, ring, *p2)
        assert orc.serialize_slice(table, wmb, hmb, ring, *planes) == pay
        assert cairo.serialize_slice(table, wmb, hmb, ring, *planes) == pay
