"""bench.py --dump-outputs and the plain / --full split: the .npy writer and
the resident-frame cap on CPU, and one small plain run on the GPU whose dumped
feeds are arithmetic-coded here and compared with the oracle's records."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _last(cairo, frames, mbs, words, seed=5):
    rng = np.random.default_rng(seed)
    last = {}
    for k, f in enumerate(frames):
        tb = np.zeros(mbs, cairo.BLOCK_DESC)
        tb["block_type"] = rng.integers(0, 8, mbs)
        tb["motion_x"] = rng.integers(-32768, 32768, mbs)
        tb["motion_y"] = rng.integers(-32768, 32768, mbs)
        tb["q_index"] = rng.integers(0, 256, mbs)
        tb["variance"] = rng.integers(-32768, 32768, mbs)
        n = words - k  # feeds of different lengths
        fw = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        fw[-1] = 0xFFFFFFFF  # the largest word survives float64
        last[f] = (tb, fw, n * 32 - 5, cairo.FEED_VALID)
    return last


def _load(path):
    return {n[:-4]: np.load(os.path.join(path, n)) for n in os.listdir(path)}


def test_dump_outputs_whole_step(cairo, tmp_path):
    """Every frame of the step fits: tables and feeds come back exactly."""
    last = _last(cairo, range(40, 46), mbs=30, words=50)
    info = bench.dump_outputs(str(tmp_path / "o"), last)
    d = _load(str(tmp_path / "o"))
    assert sorted(d) == info["arrays"] and info["frames"] == info["of"] == 6
    assert all(v.dtype in (np.float32, np.float64) for v in d.values())
    assert info["bytes"] == sum(v.nbytes for v in d.values())
    assert d["frame_index"].tolist() == list(range(40, 46))
    for i, f in enumerate(range(40, 46)):
        tb, fw, bits, status = last[f]
        for c, name in enumerate(bench.TABLE_COLUMNS):
            np.testing.assert_array_equal(d["block_table"][i, :, c].astype(np.int64), tb[name].astype(np.int64))
        np.testing.assert_array_equal(d["feed_words"][i, :fw.size].astype(np.uint32), fw)
        assert not d["feed_words"][i, fw.size:].any()
        assert (d["feed_bits"][i], d["feed_status"][i]) == (bits, status)


def test_dump_outputs_sample_is_fixed_and_bounded(cairo, tmp_path):
    """A step larger than the limit: a sample of whole frames, the same one
    every time, within the limit; an overflowed feed is dumped as no words."""
    last = _last(cairo, range(8), mbs=30, words=50)
    last[3] = (last[3][0], None, 0, cairo.FEED_OVERFLOW)
    per_frame = 30 * len(bench.TABLE_COLUMNS) * 4 + 50 * 8 + 24
    a = bench.dump_outputs(str(tmp_path / "a"), last, limit=5 * per_frame + 7)
    b = bench.dump_outputs(str(tmp_path / "b"), last, limit=5 * per_frame + 7)
    da, db = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert a["frames"] == 5 and a["of"] == 8 and a["bytes"] <= 5 * per_frame + 7
    for n in da:
        np.testing.assert_array_equal(da[n], db[n])
    picked = da["frame_index"].astype(int).tolist()
    assert picked == sorted(set(picked)) and set(picked) <= set(range(8))
    for i, f in enumerate(picked):
        fw = last[f][1]
        if fw is None:
            assert not da["feed_words"][i].any() and da["feed_status"][i] == cairo.FEED_OVERFLOW
        else:
            np.testing.assert_array_equal(da["feed_words"][i, :fw.size].astype(np.uint32), fw)


def test_dump_outputs_one_oversized_frame(cairo, tmp_path):
    """One frame alone is over the limit: its table and a prefix of its feed."""
    last = _last(cairo, [9], mbs=10, words=100)
    fixed = 10 * len(bench.TABLE_COLUMNS) * 4 + 24
    info = bench.dump_outputs(str(tmp_path / "o"), last, limit=fixed + 8 * 20)
    d = _load(str(tmp_path / "o"))
    assert info["frames"] == 1 and info["bytes"] <= fixed + 8 * 20
    np.testing.assert_array_equal(d["feed_words"][0].astype(np.uint32), last[9][1][:20])


def test_resident_frames_are_capped():
    """The default runs keep every frame distinct (the golden stream's); a
    longer run cycles a bounded pool instead of growing with --steps."""
    fb = 3840 * 2160 * 3
    assert bench.content_pool("band4", 3 * 32 + 2 * 20 * 32, fb) == 3 * 32 + 2 * 20 * 32
    assert bench.content_pool("band4", 100000, fb) == 1440
    assert bench.content_pool("band4", 100000, fb) * fb <= bench.POOL_BYTES
    assert bench.content_pool("noise", 100000, fb) == bench.NOISE_POOL
    assert bench.content_pool("static", 100000, fb) == 1
    assert bench.DUMP_BYTES <= 64 * 1000 * 1000


def test_full_is_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert (a.full, a.dump_outputs) == (True, "d")


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(orc, cairo, tmp_path):
    """A plain CIF run: the line has the timed steps it was asked for and none
    of the --full legs; the dumped frames are the last step's, and each dumped
    feed, arithmetic-coded here, is the oracle's record of that frame."""
    w, h, ring, q, _ = bench.CONFIGS["cif"]
    steps, warm, batch = 2, 1, 4
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warm), "--config", "cif", "--batch", str(batch), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert (d["steps"], d["warmup"], d["full"], d["unit"], d["dtype"]) == (steps, warm, False, "Mpix/s", "int16")
    assert d["config"]["timed_frames"] == steps * batch and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(w * h * batch / (d["ms_per_step"] * 1e-3) / 1e6, rel=1e-3)
    for leg in ("end_to_end", "host_rgb", "api_encode", "cpu_baseline", "bit_exact"):
        assert d[leg] is None, leg
    a = _load(str(out))
    nframes = (steps + warm) * batch
    assert a["frame_index"].tolist() == list(range(nframes - batch, nframes))
    assert sum(v.nbytes for v in a.values()) <= 64 * 1000 * 1000
    assert a["block_table"].shape == (batch, (w // 16) * (h // 16), len(bench.TABLE_COLUMNS))
    e = orc.OracleEncoder(ring)
    e.set_quality(q)
    for t in range(nframes):
        data, nb = e.encode(bench.content_frame("band4", w, h, t))
        if t < nframes - batch:
            continue
        i = t - (nframes - batch)
        assert a["feed_status"][i] == cairo.FEED_VALID
        bits = int(a["feed_bits"][i])
        words = a["feed_words"][i, :(bits + 31) // 32].astype(np.uint32)
        got, gbits = bench.record(cairo, w, h, ring, q, t, *cairo.serialize_feed(words, bits))
        assert gbits == nb, t
        assert orc.canonical_frame_bytes(got, gbits, False) == orc.canonical_frame_bytes(data, nb, False), t
        tb = e.block_table()
        np.testing.assert_array_equal(a["block_table"][i, :, 0].astype(np.uint32), tb["block_type"])
        np.testing.assert_array_equal(a["block_table"][i, :, 2].astype(np.int16), tb["motion_x"])
