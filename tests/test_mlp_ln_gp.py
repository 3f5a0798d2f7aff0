"""The MLP WGAN-GP with the LReLU + LayerNorm critic, zoo ``("mlp_ln", "wgan_gp")`` / alias ``ln_wgan_gp``
(models/gan.py, train/mlp_fused.py head 3), CPU only: the zoo entry, the trainer on the explicit engine,
the fused path's selection logic and the CLI round trip.  The engine's gradients of this model are checked
against autograd double backward by tests/test_engine.py (the key joins its KEYS parametrisation).
"""
import json
import os
import subprocess
import sys

import numpy as np
import torch

from hfrep.models import gan as zoo
from hfrep.train.gan_trainer import GANConfig, GANTrainer
from hfrep.train.mlp_fused import FusedMLP, _critic_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = ("mlp_ln", "wgan_gp")


def test_zoo_entry_and_alias():
    assert zoo.resolve("ln_wgan_gp") == KEY and zoo.resolve("MLP_LN_WGAN_GP") == KEY
    e = zoo.ZOO[KEY]
    assert e.loss == "wgan_gp" and e.gp_weight == 10.0 and e.n_critic == 5 and e.clip == 0.0
    # the generator and the critic of the clipped MLP WGAN: 17 635 and 14 201 parameters at (48, 35)
    G, C = e.generator(48, 35, seed=1), e.critic(48, 35, seed=2)
    w = zoo.ZOO[("mlp", "wgan")]
    assert G.count_params() == 17635 == w.generator(48, 35, seed=1).count_params()
    assert C.count_params() == 14201 == w.critic(48, 35, seed=2).count_params()
    classes = [v.legacy_class for v in zoo.ZOO.values()]
    assert len(set(classes)) == len(classes) == len(zoo.LEGACY)
    prefixes = [v.save_prefix for v in zoo.ZOO.values()]
    assert len(set(prefixes)) == len(prefixes)


def _trainer(T=6, F=5, hidden=7, B=8, **kw):
    ds = np.random.RandomState(0).rand(32, T, F).astype(np.float32)
    cfg = GANConfig(arch=KEY[0], loss=KEY[1], window=T, features=F, batch_size=B, hidden=hidden, seed=3, **kw)
    return GANTrainer(cfg, ds, device="cpu")


def test_three_cpu_iterations():
    tr = _trainer()
    assert tr._fused is None and tr.gp_weight == 10.0
    before = tr.critic.flat.clone()
    for _ in range(3):
        tr.train_step()
        rec = tr.losses()
        assert all(np.isfinite(v) for v in rec.values()), rec
        assert rec["gp"] > 0, rec
        assert abs(rec["d_loss"] - (rec["d_real"] + rec["d_fake"] + 10.0 * rec["gp"])) <= 1e-4 * max(1, abs(rec["d_loss"]))
    assert not torch.equal(before, tr.critic.flat)


def test_fused_selection_on_cpu():
    tr = _trainer()
    assert FusedMLP.decline_reason(tr) == "device is not a GPU"
    assert not FusedMLP.supported(tr)
    # the other arches are still told apart from the MLP models
    ds = np.random.RandomState(0).rand(32, 6, 5).astype(np.float32)
    lstm = GANTrainer(GANConfig(arch="lstm_ln", loss="wgan_gp", window=6, features=5, batch_size=4, hidden=7), ds)
    assert FusedMLP.decline_reason(lstm) == "not an MLP model of the zoo"


def test_head_3_views_in_model_order():
    T, F, H = 6, 32, 100
    C = zoo.ZOO[KEY].critic(T, F, H, seed=1)
    views = _critic_of(C, 3)
    assert views is not None and len(views) == 10
    assert [tuple(v.shape) for v in views] == [(F, H), (H,), (H,), (H,), (H, H), (H,), (H,), (H,), (H, 1), (1,)]
    assert [v.data_ptr() for v in views] == [v.data_ptr() for _, v in C.named_weights()]
    C.zero_grad()
    grads = _critic_of(C, 3, grad=True)
    assert [g.shape for g in grads] == [v.shape for v in views]
    assert grads[0].data_ptr() == C.flat.grad.data_ptr()
    # the affine GP critic is not this head's model
    assert _critic_of(zoo.ZOO[("mlp", "wgan_gp")].critic(T, F, H, seed=1), 3) is None


def test_cli_train_generate_round_trip(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    py = [sys.executable, "-m", "hfrep"]
    out = subprocess.run(py + ["train", "--model", "ln_wgan_gp", "--preset", "smoke", "--device", "cpu", "--epochs", "3",
                               "--quiet", "--save-dir", str(tmp_path / "gen")],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    saved = json.loads(out.stdout.strip().splitlines()[-1])["saved"]
    assert os.path.exists(saved) and os.path.basename(saved).startswith("LN_GAN_GP")
    fake = tmp_path / "fake.npy"
    out = subprocess.run(py + ["generate", "--ckpt", saved, "--n", "16", "--device", "cpu", "--out", str(fake)],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    arr = np.load(fake)
    assert arr.ndim == 3 and arr.shape[0] == 16 and np.isfinite(arr).all()
