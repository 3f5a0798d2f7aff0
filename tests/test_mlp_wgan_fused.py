"""Structure matcher of the fused clipped-WGAN path (train/mlp_fused.py:_clip_critic_lists), CPU only.

The fused critic kernels hard-code the reference critic of GAN/WGAN.py:147-158 (Dense(linear) ->
LeakyReLU(0.2) -> LayerNorm(eps 1e-3), twice, then Dense(1)); the matcher must hand them exactly that
model's ten parameter views in model order and decline everything else.
"""
import pytest
import torch

from hfrep.models import gan as zoo
from hfrep.models.layers import Dense, LayerNormalization, LeakyReLU, Sequential
from hfrep.train.mlp_fused import _clip_critic_lists

T, F, H = 6, 32, 100


def _clip(alpha=0.2, eps=1e-3, act=None, head_units=1, bias=True):
    ln = lambda: LayerNormalization(epsilon=eps)  # noqa: E731
    return Sequential([Dense(H, act, use_bias=bias), LeakyReLU(alpha), ln(), Dense(H), LeakyReLU(alpha), ln(),
                       Dense(head_units)], (T, F), name="critic", seed=3)


def test_matcher_returns_the_ten_views_in_model_order():
    C = zoo.ZOO[("mlp", "wgan")].critic(T, F, H, seed=1)
    views = _clip_critic_lists(C)
    assert views is not None and len(views) == 10
    assert [tuple(v.shape) for v in views] == [(F, H), (H,), (H,), (H,), (H, H), (H,), (H,), (H,), (H, 1), (1,)]
    # model order: the same storage, in the order of the model's own weight list
    named = [v for _, v in C.named_weights()]
    assert [v.data_ptr() for v in views] == [v.data_ptr() for v in named]
    assert [v.data_ptr() for v in views] == sorted(v.data_ptr() for v in views)
    # gamma = 1, beta = 0 at initialisation identify the LayerNorm slots
    for i in (2, 6):
        assert torch.equal(views[i], torch.ones_like(views[i])) and torch.equal(views[i + 1], torch.zeros_like(views[i]))
    C.zero_grad()
    grads = _clip_critic_lists(C, grad=True)
    assert [g.shape for g in grads] == [v.shape for v in views]
    assert grads[0].data_ptr() == C.flat.grad.data_ptr()


def test_matcher_accepts_the_hand_built_reference_critic():
    assert _clip_critic_lists(_clip()) is not None


@pytest.mark.parametrize("loss", ["gan", "wgan_gp"])
def test_matcher_declines_the_other_mlp_critics(loss):
    assert _clip_critic_lists(zoo.ZOO[("mlp", loss)].critic(T, F, H, seed=1)) is None


@pytest.mark.parametrize("kw", [dict(alpha=0.3), dict(eps=1e-5), dict(act="sigmoid"), dict(head_units=2),
                                dict(bias=False)])
def test_matcher_declines_a_changed_clip_critic(kw):
    assert _clip_critic_lists(_clip(**kw)) is None


def test_matcher_declines_the_generator():
    assert _clip_critic_lists(zoo.ZOO[("mlp", "wgan")].generator(T, F, H, seed=1)) is None
