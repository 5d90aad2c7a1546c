"""bench.py on the GPU, in process and at two stripes per step: a plain run
times exactly --steps steps and measures nothing else, --dump-outputs writes
the parity of the last timed step (checked against the oracle through the
exact row sums, and run to run), and --full fills the other figures in."""
import json
import os
import sys

import numpy as np
import pytest

from oracle import orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRAS = ("unpadded_rows", "single_stripe", "cpu_baseline", "other_workloads", "host_resident", "calibration")
K, P, S, B, PAD = 128, 32, 1 << 20, 2, 3584


@pytest.fixture(scope="module")
def bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench as b

    return b


def run_bench(bench, monkeypatch, capsys, *args):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", *args])
    capsys.readouterr()
    bench.main()
    return json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])


def test_plain_run_times_the_steps_and_dumps_the_parity(bench, monkeypatch, capsys, tmp_path):
    import torch

    from reedsolomon16_amd.codec import ReedSolomon

    launches = []
    encode = ReedSolomon.encode_dev_batch
    monkeypatch.setattr(ReedSolomon, "encode_dev_batch",
                        lambda self, slab, stream=None: (launches.append(tuple(slab.shape)), encode(self, slab, stream))[1])
    res = [run_bench(bench, monkeypatch, capsys, "--steps", "3", "--warmup", "1", "--stripes", str(B),
                     "--dump-outputs", str(tmp_path / d)) for d in ("a", "b")][0]
    # a plain run launches its warm-up and its timed steps, nothing else
    assert launches == [(B, K + P, S)] * (2 * (1 + 3))
    assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0
    assert res["unit"] == "GiB/s" and res["higher_is_better"] is True
    # value is the data bytes of the timed steps over their wall time
    assert res["value"] == pytest.approx(B * K * S / (res["ms_per_step"] * 1e-3) / 2**30, rel=1e-3)
    assert all(res[key] is None for key in EXTRAS)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["parity_row_sums.npy", "parity_sample.npy"] == sorted(os.listdir(tmp_path / "b"))
    sums, sample = (np.load(tmp_path / "a" / f) for f in files)
    assert sums.dtype == np.float64 and sums.shape == (B, P)
    assert sample.dtype == np.float32 and sample.shape[:2] == (B, P) and 2 <= sample.shape[2] <= S
    assert sums.nbytes + sample.nbytes <= 64 << 20
    for f in files:  # same arguments, same inputs, same outputs
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
    # the bench's seeded input, regenerated: the dumped row sums are the oracle's parity's
    g = torch.Generator(device="cuda")
    g.manual_seed(0x5EED)
    RS = S + PAD
    buf = torch.randint(0, 256, (B * (K + P) * RS,), dtype=torch.uint8, device="cuda", generator=g)
    slab = buf.as_strided((B, K + P, S), ((K + P) * RS, RS, 1))
    for j in range(B):
        ref = orc.encode(16, K, P, slab[j, :K].cpu().numpy())
        assert np.array_equal(sums[j], ref.sum(axis=1, dtype=np.int64).astype(np.float64)), f"stripe {j}"
        assert np.array_equal(sample[j, :, 0], ref[:, 0]) and np.array_equal(sample[j, :, -1], ref[:, -1])


def test_dump_sample_is_bounded_and_keeps_the_corners(bench, monkeypatch, tmp_path):
    import torch

    monkeypatch.setattr(bench, "DUMP_SAMPLE_ELEMS", 4 * 3 * 50)
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    buf = torch.randint(0, 256, (11 * 9 * 1064,), dtype=torch.uint8, device="cuda", generator=g)
    parity = buf.as_strided((11, 9, 1000), (9 * 1064, 1064, 1))[:, 6:]  # strided rows, as the bench holds them
    bench.dump_outputs(torch, str(tmp_path), parity, 0, 1)
    host = parity.cpu().numpy()
    sums, sample = np.load(tmp_path / "parity_row_sums.npy"), np.load(tmp_path / "parity_sample.npy")
    assert np.array_equal(sums, host.sum(axis=2, dtype=np.int64))
    assert sample.shape[1] == 3 and sample.shape[0] <= 8 and sample.size <= 8 * 3 * 50
    for i, j in ((0, 0), (0, -1), (-1, 0), (-1, -1)):
        assert np.array_equal(sample[i, :, j], host[i, :, j])
    # a parity that fits the sample is dumped whole
    monkeypatch.setattr(bench, "DUMP_SAMPLE_ELEMS", 8 << 20)
    bench.dump_outputs(torch, str(tmp_path), parity[:5], 0, 1)
    assert np.array_equal(np.load(tmp_path / "parity_sample.npy"), host[:5])


def test_full_run_fills_the_other_figures(bench, monkeypatch, capsys):
    res = run_bench(bench, monkeypatch, capsys, "--steps", "2", "--warmup", "1", "--stripes", str(B), "--full",
                    "--no-other", "--no-host", "--cpu-seconds", "0.2", "--cpu-threads", "2")
    assert res["steps"] == 2 and res["ms_per_step"] > 0
    assert res["unpadded_rows"]["kernel_ms"] > 0 and res["single_stripe"]["kernel_ms"] > 0
    assert res["cpu_baseline"]["value"] > 0
