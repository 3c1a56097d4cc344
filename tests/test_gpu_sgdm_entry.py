"""The training entry with the fused momentum / weight-decay update (`training_loop.fused_momentum`):
a tiny `train` run built like tests/test_gpu_entry.py's, with train.momentum = 0.9 and
train.wd = 5e-4, two epochs of two steps; the checkpoints' 'optimizer' entry carries the
engine's momentum buffers as torch.optim.SGD state, as the reference's checkpoints do
(src/utils.py:107-115).  Without the opt-in the same call is refused as before."""
import os

import pytest
import torch

from test_gpu_entry import GUIDED, _dataset, _run

pytestmark = pytest.mark.gpu

SGDM = GUIDED.replace("train.wd=0.0", "train.wd=5e-4").replace("train.momentum=0", "train.momentum=0.9")


def test_train_with_fused_momentum_checkpoints_the_buffers(tmp_path):
    from greedy_multimodal_learning_amd.model import MMTM_MVCNN
    from greedy_multimodal_learning_amd.train import train
    assert "train.wd=5e-4" in SGDM and "train.momentum=0.9" in SGDM
    data = str(tmp_path / "data")
    _dataset(data, n_train=10)  # 8 training samples (80 % of 10) at batch 4 -> 2 steps
    ds = f"\nget_mvdcndata.root_dir='{data}'\n"
    save = str(tmp_path / "sgdm")
    H = _run(train, SGDM + ds + "training_loop.fused_momentum=True\n", save)
    assert len(H["loss"]) == 2 and all(len(d) == 2 for d in H["d_BDR"])
    shapes = [tuple(p.shape) for p in MMTM_MVCNN(num_views=2, pretraining=False).parameters()]
    for f in ("model_best_val.pt", "model_last_epoch.pt"):
        ck = torch.load(os.path.join(save, f), weights_only=True)
        opt = ck["optimizer"]
        group = opt["param_groups"][0]
        assert group["momentum"] == 0.9 and group["weight_decay"] == 5e-4 and group["lr"] == 0.1
        assert group["params"] == list(range(len(shapes)))
        assert sorted(opt["state"]) == group["params"]
        for i, shape in enumerate(shapes):
            b = opt["state"][i]["momentum_buffer"]
            assert tuple(b.shape) == shape, i
            assert b.dtype == torch.float32 and bool(torch.isfinite(b).all()) and bool(b.any()), i
    with pytest.raises(NotImplementedError):
        _run(train, SGDM + ds + "training_loop.fused_momentum=False\n", str(tmp_path / "refused"))
    with pytest.raises(NotImplementedError):
        _run(train, SGDM + ds, str(tmp_path / "refused"))
