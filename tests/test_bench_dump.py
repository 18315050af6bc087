"""CPU: bench.py --dump-outputs -- which arrays of a step are written, in what format, within the size budget, and the
same elements from run to run."""
import numpy as np
import torch

import bench


def _step(B=2, S=3, H=40, W=44, nq=5, streams=2, world=2):
    g = torch.Generator().manual_seed(11)
    batch_outs = []
    for _ in range(streams):
        batch_outs.append({"pose_enc": torch.randn(B, S, 9, generator=g),
                           "pose_enc_list": [torch.randn(B, S, 9, generator=g) for _ in range(4)],
                           "depth": torch.randn(B, S, H, W, 1, generator=g),
                           "world_points": torch.randn(B, S, H, W, 3, generator=g),
                           "track": torch.randn(B, S, nq, 2, generator=g),
                           "images": torch.rand(B, S, 3, H, W, generator=g)})
    n = streams * B
    # this rank's joints and cameras of the step, and (as under N ranks) the gathered ones of every rank's shard
    out = {"joints3d_local": torch.randn(n, 17, 3, generator=g), "E_local": torch.randn(n, S, 3, 4, generator=g),
           "K_local": torch.randn(n, S, 3, 3, generator=g).double()}
    for k in ("joints3d", "E", "K"):
        out[k] = torch.cat([out[k + "_local"]] * world)
    return batch_outs, out


def test_step_outputs_cover_every_batch_of_this_ranks_time_steps():
    batch_outs, out = _step()
    arrays = bench.step_outputs(batch_outs, out)
    assert sorted(arrays) == ["E", "K", "depth", "joints3d", "pose_enc", "pose_enc_list", "track", "world_points"]
    assert torch.equal(arrays["depth"], torch.cat([o["depth"] for o in batch_outs]))
    assert arrays["pose_enc_list"].shape == (4, 4, 3, 9)
    assert torch.equal(arrays["pose_enc_list"][2, 2:], batch_outs[1]["pose_enc_list"][2])
    for k in ("joints3d", "E", "K"):   # the same time steps as the model outputs, not the gathered shards
        assert arrays[k] is out[k + "_local"] and arrays[k].shape[0] == arrays["pose_enc"].shape[0]


def test_dump_outputs_budget_format_and_repeatability(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 200_000)     # small budget: depth and world_points get sampled
    batch_outs, out = _step()
    arrays = bench.step_outputs(batch_outs, out)
    d1 = bench.dump_outputs(tmp_path / "a", arrays)
    d2 = bench.dump_outputs(tmp_path / "b", arrays)
    assert d1["arrays"] == d2["arrays"] and d1["bytes"] <= 200_000
    share = 200_000 // len(arrays)
    total = 0
    for name, t in arrays.items():
        a = np.load(tmp_path / "a" / f"{name}.npy")
        assert a.tobytes() == np.load(tmp_path / "b" / f"{name}.npy").tobytes(), name
        assert a.dtype == (np.float64 if t.dtype == torch.float64 else np.float32), name
        total += a.nbytes
        entry = d1["arrays"][name]
        assert entry["shape"] == list(t.shape)
        if entry["sampled_elements"] is None:
            assert np.array_equal(a, t.numpy()), name
        else:
            # the documented sampling rule: the same elements for the same shape, whatever build wrote them
            idx = np.unique(np.random.default_rng(bench.DUMP_SEED).integers(0, t.numel(), size=share // a.itemsize))
            assert a.shape == (entry["sampled_elements"],) == idx.shape and 0 < a.size < t.numel()
            assert np.array_equal(a, t.reshape(-1).numpy()[idx].astype(a.dtype)), name
    assert d1["arrays"]["depth"]["sampled_elements"] and d1["arrays"]["world_points"]["sampled_elements"]
    assert d1["arrays"]["pose_enc"]["sampled_elements"] is None
    assert total == d1["bytes"]
