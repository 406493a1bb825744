"""CPU checks of what `bench.py --gpus N` hands each rank it starts (no GPU, no process is spawned): the driver will run
that command on an 8-GPU node some day without anybody watching -- the environment of the ranks must be right by
construction.  Partitioning the path keeps: image i -> rank i mod N; counts, then padded records."""
import importlib.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("n", [2, 4, 8])
def test_rank_envs(bench, n):
    base = {"PATH": "/usr/bin", "RANK": "7", "WORLD_SIZE": "99", "SOMETHING": "kept"}
    envs = bench.rank_envs(n, 29511, base)
    assert len(envs) == n
    assert [e["RANK"] for e in envs] == [str(r) for r in range(n)]
    assert [e["LOCAL_RANK"] for e in envs] == [str(r) for r in range(n)]          # one node: rank r drives GPU r
    for e in envs:
        assert e["WORLD_SIZE"] == str(n) and e["LOCAL_WORLD_SIZE"] == str(n)
        assert e["MASTER_ADDR"] == "127.0.0.1" and e["MASTER_PORT"] == "29511"    # one rendezvous for all of them
        assert e["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"                             # dmabuf IPC, or RCCL cannot share buffers
        assert e["OMP_NUM_THREADS"] == "1"
        assert e["SOMETHING"] == "kept" and e["PATH"] == "/usr/bin"
    assert base["RANK"] == "7"                                                    # the caller's mapping is not touched
    # the caller's own choices win where they are choices
    envs = bench.rank_envs(n, 1, dict(base, OMP_NUM_THREADS="4", HSA_ENABLE_IPC_MODE_LEGACY="1"))
    assert all(e["OMP_NUM_THREADS"] == "4" and e["HSA_ENABLE_IPC_MODE_LEGACY"] == "1" for e in envs)


@pytest.mark.parametrize("n", [1, 2, 4, 8])
def test_every_frame_has_exactly_one_owner(n):
    from sift_pyocl_amd.batch import shard_indices
    for frames in (64, 7, 1, 0):
        owned = [shard_indices(frames, r, n) for r in range(n)]
        assert sorted(i for o in owned for i in o) == list(range(frames))
        for r, o in enumerate(owned):
            assert all(i % n == r for i in o)                                     # image i -> rank i mod N


def test_default_flags_are_the_driver_contract(bench, monkeypatch):
    """`python bench.py` alone must mean N = 1 and a K / W that finish in minutes; --gpus / --steps / --warmup parse."""
    import argparse
    seen = {}
    real = argparse.ArgumentParser.parse_args

    def spy(self, *a, **k):
        ns = real(self, *a, **k)
        seen["ns"] = ns
        raise SystemExit(0)
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", spy)
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    with pytest.raises(SystemExit):
        bench.main()
    assert seen["ns"].gpus == 1 and 1 <= seen["ns"].steps <= 100 and 0 <= seen["ns"].warmup <= 20 and seen["ns"].config == "c2"
    assert not seen["ns"].full and not seen["ns"].dump_outputs          # a plain run measures the headline only
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8", "--steps", "5", "--warmup", "2"])
    with pytest.raises(SystemExit):
        bench.main()
    assert (seen["ns"].gpus, seen["ns"].steps, seen["ns"].warmup) == (8, 5, 2)


def test_dump_outputs_layout(bench, tmp_path, monkeypatch):
    """--dump-outputs: float32 / float64 arrays, records sorted within a frame (the library's order is not specified), so
    that the same records in another order give the same files; above DUMP_MAX_ROWS a fixed sample of rows."""
    from sift_pyocl_amd import SiftPlan
    rng = np.random.default_rng(4)
    frames = []
    for n in (300, 0, 170):
        k = np.zeros(n, SiftPlan.dtype_kp)
        for f in ("x", "y", "scale", "angle"):
            k[f] = rng.random(n, dtype=np.float32) * 100
        k["desc"] = rng.integers(0, 256, (n, 128), dtype=np.uint8)
        frames.append(k)

    def dump(where, frames):
        rows = bench.dump_outputs(str(where), frames)
        return rows, {name: np.load(os.path.join(str(where), name + ".npy")) for name in ("keypoints", "descriptors", "frame", "counts")}

    rows, a = dump(tmp_path / "a", frames)
    assert rows == 470 and a["keypoints"].shape == (470, 4) and a["descriptors"].shape == (470, 128) and a["frame"].shape == (470,)
    assert a["keypoints"].dtype == a["descriptors"].dtype == a["frame"].dtype == np.float32 and a["counts"].dtype == np.float64
    assert a["counts"].tolist() == [300, 0, 170] and (np.diff(a["frame"]) >= 0).all()
    first = frames[0]
    got = {tuple(r) for r in np.concatenate([a["keypoints"][:300], a["descriptors"][:300]], axis=1)}
    want = {tuple(r) for r in np.concatenate([np.stack([first[f] for f in ("x", "y", "scale", "angle")], axis=1),
                                              first["desc"].astype(np.float32)], axis=1)}
    assert got == want
    _, b = dump(tmp_path / "b", [k[rng.permutation(len(k))] for k in frames])
    assert all(np.array_equal(a[n], b[n]) for n in a)
    monkeypatch.setattr(bench, "DUMP_MAX_ROWS", 100)
    rows, c = dump(tmp_path / "c", frames)
    _, d = dump(tmp_path / "d", [k[rng.permutation(len(k))] for k in frames])
    assert rows == 100 and c["keypoints"].shape == (100, 4) and c["counts"].tolist() == [300, 0, 170]
    assert all(np.array_equal(c[n], d[n]) for n in c)
