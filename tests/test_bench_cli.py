"""bench.py's command line: --full is off by default, and --dump-outputs
writes the last step's loss and a fixed sample of the parameter arena as
float32 .npy files, the same elements on every call.

Tensors here stay far below torch's parallel grain size: a test process whose
OpenMP pool is up cannot fork test_dist_gloo's ranks afterwards."""
import types

import numpy as np
import torch

import bench


def test_full_and_dump_outputs_are_opt_in(monkeypatch):
    import argparse
    seen = {}
    real = argparse.ArgumentParser.parse_args

    def grab(self, *a, **k):
        seen["args"] = real(self, *a, **k)
        raise SystemExit(0)  # the options only: nothing of the run itself

    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", grab)
    for argv, full, dump in ((["--gpus", "1", "--steps", "7", "--warmup", "2"], False, None),
                             (["--full", "--dump-outputs", "d"], True, "d")):
        monkeypatch.setattr("sys.argv", ["bench.py"] + argv)
        try:
            bench.main()
        except SystemExit:
            pass
        assert seen["args"].full is full and seen["args"].dump_outputs == dump
    assert seen["args"].steps == 10 and seen["args"].warmup == 3  # the defaults


def test_dump_outputs_files(tmp_path, monkeypatch):
    assert 4 * (bench.DUMP_SAMPLE + 1) <= 64 << 20  # the shipped sample size, in bytes
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    n = 3 * bench.DUMP_SAMPLE + 17
    flat = torch.arange(n, dtype=torch.float32) * 0.5
    eng = types.SimpleNamespace(arena=types.SimpleNamespace(flat=flat))
    loss = torch.tensor(2.5, dtype=torch.bfloat16)
    bench.dump_outputs(str(tmp_path / "a"), eng, loss)
    bench.dump_outputs(str(tmp_path / "b"), eng, loss)
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["loss.npy", "params_sample.npy"]
    la, pa = np.load(tmp_path / "a" / "loss.npy"), np.load(tmp_path / "a" / "params_sample.npy")
    assert la.dtype == np.float32 and la.shape == (1,) and la[0] == 2.5
    assert pa.dtype == np.float32 and pa.shape == (bench.DUMP_SAMPLE,)
    # arena elements (value = 0.5 * offset), in arena order, spread over the whole arena
    off = pa.astype(np.float64) * 2
    assert np.all(off == np.round(off)) and np.all(np.diff(off) >= 0)
    assert off[0] < 0.02 * n and off[-1] > 0.98 * n
    assert np.array_equal(pa, np.load(tmp_path / "b" / "params_sample.npy"))  # the same sample every time
    # an arena smaller than the sample: never past its end
    small = types.SimpleNamespace(arena=types.SimpleNamespace(flat=torch.ones(5)))
    bench.dump_outputs(str(tmp_path / "c"), small, loss)
    assert np.load(tmp_path / "c" / "params_sample.npy").shape == (5,)
