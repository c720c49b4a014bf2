"""bench.py's multi-GPU record must be self-proving: N ranks on fewer than N devices are
refused unless --rehearsal is given, and the identities that go into the line count distinct devices by UUID.
A plain run only times the steps (everything else is behind --full), --steps is the number of timed steps, and
--dump-outputs writes what the last timed step handed back."""
import argparse
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_ranks_sharing_a_gpu_are_refused_without_rehearsal(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    with pytest.raises(SystemExit) as e:
        bench.pick_device(argparse.Namespace(rehearsal=False), 1, 2)
    assert "rehearsal" in str(e.value)
    assert bench.pick_device(argparse.Namespace(rehearsal=True), 1, 2) == 0       # wraps, labelled by the caller
    assert bench.pick_device(argparse.Namespace(rehearsal=False), 0, 1) == 0
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 8)
    assert [bench.pick_device(argparse.Namespace(rehearsal=False), r, 8) for r in range(8)] == list(range(8))


def test_devices_seen_counts_distinct_uuids():
    bench = _bench()
    a = {"rank": 0, "host": "h", "uuid": "GPU-aa", "device": 0, "name": "x"}
    b = dict(a, rank=1)                      # a second rank on the SAME device
    c = dict(a, rank=1, uuid="GPU-bb", device=1)
    assert bench.devices_seen([a, b]) == 1
    assert bench.devices_seen([a, c]) == 2
    assert bench.devices_seen([a, dict(c, host="other", uuid="GPU-aa")]) == 2   # same UUID text, another host


def test_self_launch_refuses_before_spawning(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    called = []
    monkeypatch.setattr(bench.subprocess, "call", lambda cmd: called.append(cmd) or 0)
    with pytest.raises(SystemExit) as e:
        bench.self_launch_if_needed(argparse.Namespace(gpus=2, rehearsal=False))
    assert "rehearsal" in str(e.value) and not called


def _args(bench, monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse_args()


def test_steps_and_full_flags(monkeypatch):
    bench = _bench()
    a = _args(bench, monkeypatch, "--gpus", "1", "--steps", "5", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (5, 2, False, None)
    assert _args(bench, monkeypatch, "--full").full
    assert (_args(bench, monkeypatch).steps, _args(bench, monkeypatch).warmup) == (64, 8)
    # the modes' own defaults apply only where --steps / --warmup are not given
    assert (_args(bench, monkeypatch, "--mode", "tp").steps, _args(bench, monkeypatch, "--mode", "prefill").steps) == (32, 3)
    assert _args(bench, monkeypatch, "--mode", "tp", "--steps", "64").steps == 64
    assert _args(bench, monkeypatch, "--mode", "prefill", "--steps", "64", "--warmup", "8").warmup == 8
    for bad in (["--steps", "0"], ["--mode", "serve", "--dump-outputs", "d"]):
        with pytest.raises(SystemExit):
            _args(bench, monkeypatch, *bad)


def test_dump_outputs_writes_ids_and_a_seeded_logit_sample(tmp_path):
    from scratchpad_amd.llama import LogitsProcessorOutput
    bench = _bench()
    g = torch.Generator().manual_seed(1)
    logits = torch.randn(6, 20000, generator=g)
    ids = torch.randint(0, 20000, (6,), generator=g)
    bench.dump_outputs(str(tmp_path / "a"), LogitsProcessorOutput(next_token_logits=logits), ids)
    bench.dump_outputs(str(tmp_path / "b"), LogitsProcessorOutput(next_token_logits=logits.clone()), ids)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["next_token_ids.npy", "next_token_logits_sample.npy", "next_token_logits_sample_columns.npy"]
    got = {n: np.load(tmp_path / "a" / n) for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    cols = got["next_token_logits_sample_columns.npy"].astype(np.int64)
    assert len(cols) == 8192 and (np.diff(cols) > 0).all() and cols.max() < 20000
    np.testing.assert_array_equal(got["next_token_ids.npy"], ids.numpy())
    np.testing.assert_array_equal(got["next_token_logits_sample.npy"], logits.numpy()[:, cols])
    for n in names:                                     # the sample is fixed: same columns, same file
        np.testing.assert_array_equal(got[n], np.load(tmp_path / "b" / n))


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_full_run_adds_the_rest(tmp_path):
    """bench.py at toy size, plain and with --full: the same timed path (same dumped outputs), the plain line
    without the figures that take runs of their own."""
    lines = {}
    for kind in ("plain", "full"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
               "--layers", "2", "--bs", "8", "--ctx", "300", "--no-cpu-baseline",
               "--dump-outputs", str(tmp_path / kind)] + (["--full"] if kind == "full" else [])
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert res.returncode == 0, res.stderr[-2000:]
        lines[kind] = json.loads(res.stdout.strip().splitlines()[-1])
    plain, full = lines["plain"], lines["full"]
    for line in (plain, full):
        assert line["metric"] == "decode_tokens_per_sec" and line["steps"] == 3 and line["ms_per_step"] > 0
        assert abs(line["value"] - 8 * 1e3 / line["ms_per_step"]) <= 0.01 * line["value"]
    assert "roofline" not in plain and "roofline" in full
    ids = np.load(tmp_path / "plain" / "next_token_ids.npy")
    assert ids.shape == (8,) and (ids == np.round(ids)).all()
    assert np.load(tmp_path / "plain" / "next_token_logits_sample.npy").shape == (8, 8192)
    for name in os.listdir(tmp_path / "plain"):
        np.testing.assert_array_equal(np.load(tmp_path / "plain" / name), np.load(tmp_path / "full" / name), err_msg=name)
