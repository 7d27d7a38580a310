"""nano_vs_slam_amd.train_ops without a device: the layer calls are defined once and every old name is that object, the five
trainers share one Adam core (``AdamTrainer``), and the trainer modules depend on each other only where they must."""
import types

import pytest
import torch

from nano_vs_slam_amd import depth_training as dt, keypoint_training as kt, seg_training as st, train_ops as ops
from nano_vs_slam_amd import vlad_training as vt, vpr_head_training as ht

CBR = ("cbr_forward", "cbr_backward", "bn_vectors", "MIN_CH", "MAX_CH", "LEAKY_SLOPE")
OLD_HOMES = {
    vt: ("adam_step",),
    ht: CBR + ("cbr_forward_batch", "cbr_backward_batch", "dropout2d_scale", "adam_step"),
    st: CBR + ("conv_bias_forward", "conv_bias_backward", "maxpool2_forward", "maxpool2_backward", "shuffle_cat_forward",
               "shuffle_cat_backward", "adam_step"),
    kt: CBR + ("conv_bias_forward", "conv_bias_backward", "shuffle_cat_forward", "shuffle_cat_backward", "adam_step"),
}


def test_old_names_are_train_ops_objects():
    for module, names in OLD_HOMES.items():
        for name in names:
            assert getattr(module, name) is getattr(ops, name), (module.__name__, name)
    for name in ("adam_step", "cbr_forward", "cbr_backward", "cbr_forward_batch", "cbr_backward_batch", "dropout2d_scale", "bn_vectors",
                 "conv_bias_forward", "conv_bias_backward", "maxpool2_forward", "maxpool2_backward", "shuffle_cat_forward",
                 "shuffle_cat_backward", "_is_device", "_f32_maps", "_check_cbr", "_check_slope", "_check_drop", "_check_conv_bias"):
        assert getattr(ops, name).__module__ == ops.__name__, name


def _trainers():
    """-> [(trainer, its parameters in update order)]: the five, on CPU models (no step is run)."""
    from nano_vs_slam_amd.kp2dtiny.models.kp2dtiny import KP2DTinyV2, get_config, tiny_factory
    model = tiny_factory("S", 28)
    dense = KP2DTinyV2(**get_config("S"), nClasses=19, depth=True)
    vlad = vt.NetVLADTrainer(model)
    out = [(vlad, [vlad.layer.conv.weight, vlad.layer.centroids])]
    for t in (ht.VPRHeadTrainer(model), st.SegHeadTrainer(dense), dt.DepthHeadTrainer(dense, train="last"), kt.KeypointHeadTrainer(model)):
        out.append((t, t.parameters()))
    return out


def test_trainers_share_the_adam_core():
    trainers = _trainers()
    assert [type(t).__name__ for t, _ in trainers] == ["NetVLADTrainer", "VPRHeadTrainer", "SegHeadTrainer", "DepthHeadTrainer",
                                                       "KeypointHeadTrainer"]
    for t, params in trainers:
        assert isinstance(t, ops.AdamTrainer)
        assert type(t)._apply is ops.AdamTrainer._apply and type(t)._moments is ops.AdamTrainer._moments
        assert type(t)._check_contiguous is ops.AdamTrainer._check_contiguous
        assert t.steps == 0 and t._state == {} and (t.lr, t.betas, t.eps) == (1e-4, (0.9, 0.999), 1e-8)
        assert len(params) == {"NetVLADTrainer": 2, "VPRHeadTrainer": 11, "SegHeadTrainer": 26, "DepthHeadTrainer": 2,
                               "KeypointHeadTrainer": 20}[type(t).__name__]


def test_apply_steps_once_and_updates_every_parameter_in_order(monkeypatch):
    calls = []

    def record(param, grad, exp_avg, exp_avg_sq, step, lr, betas, eps):
        calls.append((param.data_ptr(), tuple(grad.shape), exp_avg, exp_avg_sq, step, lr, betas, eps))

    monkeypatch.setattr(ops, "adam_step", record)
    for t, params in _trainers():
        grads = [torch.zeros(p.numel()) for p in params]            # flat: _apply views a gradient as its parameter
        versions = [p._version for p in params]
        for step in (1, 2):
            del calls[:]
            t._apply(params, grads)
            assert t.steps == step
            assert [c[0] for c in calls] == [p.data_ptr() for p in params]
            assert [c[1] for c in calls] == [tuple(p.shape) for p in params]
            assert all(c[4:] == (step, t.lr, t.betas, t.eps) for c in calls)
            for p, c in zip(params, calls):
                assert c[2] is t._moments(p)[0] and c[3] is t._moments(p)[1]
        assert [p._version for p in params] == [v + 2 for v in versions]      # the engine watches the parameters' versions


def test_moments_are_lazy_and_follow_the_shape():
    t = ops.AdamTrainer()
    t._init_adam(1e-3, (0.9, 0.99), 1e-8)
    p = torch.nn.Parameter(torch.ones(3, 4))
    assert t._state == {}
    m, v = t._moments(p)
    assert m.shape == v.shape == p.shape and not m.any() and not v.any() and m is not v
    m.add_(1.0)
    assert t._moments(p)[0] is m and list(t._state) == [id(p)]
    p.data = torch.ones(5)
    m2, v2 = t._moments(p)
    assert m2 is not m and m2.shape == v2.shape == (5,) and not m2.any() and list(t._state) == [id(p)]


def test_settings_are_refused_with_the_trainers_prefix():
    class T(ops.AdamTrainer):
        _WHO = "T"

    for kw in ({"lr": -1.0}, {"betas": (1.0, 0.999)}, {"betas": (0.9, -0.1)}, {"eps": -1e-8}, {"margin": -0.1}):
        args = {"lr": 1e-4, "betas": (0.9, 0.999), "eps": 1e-8, **kw}
        with pytest.raises(ValueError, match="^T: lr .*betas .*eps "):
            T()._init_adam(**args)
    with pytest.raises(ValueError, match="^T: lr 0.1, margin -1, betas"):
        T()._init_adam(0.1, (0.9, 0.999), 1e-8, margin=-1)
    p = torch.nn.Parameter(torch.ones(3, 4).t())
    with pytest.raises(ValueError, match="^T: the head's parameters must be contiguous$"):
        T()._check_contiguous([p], "the head's")


def test_trainer_modules_import_only_what_they_need():
    def modules_of(module):
        return {v.__name__.rsplit(".", 1)[-1] for v in vars(module).values() if isinstance(v, types.ModuleType)}

    def taken_from(module, source):
        return {k for k, v in vars(module).items() if getattr(v, "__module__", None) == source.__name__}

    trainer_modules = {"vlad_training", "vpr_head_training", "seg_training", "depth_training", "keypoint_training"}
    for module in (vt, ht, st, dt, kt):
        assert not modules_of(module) & trainer_modules, module.__name__      # no trainer module reaches into another as a whole
    assert not modules_of(ops) & trainer_modules and not any(taken_from(ops, m) for m in (vt, ht, st, dt, kt))
    assert taken_from(dt, st) == {"_DenseHeadTrainer"} and not taken_from(kt, st)
    assert taken_from(ht, vt) == {"_check_layer", "_vlad_scratch", "netvlad_backward", "netvlad_forward", "triplet_margin_loss"}
    for module in (vt, st, dt, kt):
        assert not taken_from(module, ht), module.__name__
    for module in (st, dt, kt):
        assert not taken_from(module, vt), module.__name__
