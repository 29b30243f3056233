"""Group norm off the GPU: the torch composition, the slim facade, the norm='group' ResNets, the trainer's flags."""
import pytest
import torch

from distributed_tensorflow_models_amd import trainer
from distributed_tensorflow_models_amd.compat import slim
from distributed_tensorflow_models_amd.engine import TrainStep
from distributed_tensorflow_models_amd.models import nets_factory
from distributed_tensorflow_models_amd.models.layers import tf_variables
from distributed_tensorflow_models_amd.ops.groupnorm import group_norm


def test_torch_composition_against_a_float64_loop():
    N, H, W, C, G, eps = 2, 3, 3, 16, 4, 1e-6
    torch.manual_seed(0)
    x, gamma, beta = torch.randn(N, H, W, C) * 2 + 3, torch.rand(C) + 0.5, torch.randn(C)
    want = torch.empty(N, H, W, C, dtype=torch.float64)
    cg = C // G
    for n in range(N):
        for g in range(G):
            v = x[n, :, :, g * cg:(g + 1) * cg].double()
            mean = v.sum() / v.numel()
            var = ((v - mean) ** 2).sum() / v.numel()
            for c in range(g * cg, (g + 1) * cg):
                want[n, :, :, c] = (x[n, :, :, c].double() - mean) / (var + eps).sqrt() * gamma[c].double() + beta[c].double()
    torch.testing.assert_close(group_norm(x, G, gamma, beta, eps).double(), want, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(group_norm(x, G, gamma, beta, eps, relu=True).double(), want.clamp(min=0), rtol=1e-5,
                               atol=1e-5)
    with pytest.raises(ValueError):
        group_norm(x, 3)


def test_slim_group_norm_and_layer_norm_variables():
    slim.reset()
    x = torch.randn(2, 4, 4, 64)
    slim.group_norm(x)
    assert sorted(v.tf_name for v in slim.get_variables()) == ["GroupNorm/beta", "GroupNorm/gamma"]
    with pytest.raises(ValueError):
        slim.group_norm(torch.randn(2, 4, 4, 48), groups=32)
    slim.reset()
    y = slim.layer_norm(x)
    assert sorted(v.tf_name for v in slim.get_variables()) == ["LayerNorm/beta", "LayerNorm/gamma"]
    torch.testing.assert_close(y, group_norm(x, 1, eps=1e-12))
    slim.reset()


def test_group_norm_cifar_resnet_names_and_one_cpu_step():
    torch.manual_seed(0)
    m = nets_factory.build("cifar10_resnet_v2", 10, resnet_size=8, norm="group", norm_groups=8)
    names = [n for n, _, _, _ in tf_variables(m)]
    assert not any("moving_" in n or "batch_normalization" in n for n in names)
    norm_names = [n for n in names if "normalization" in n]
    assert len(norm_names) == 2 * 7  # bn1 + bn2 of three blocks, and the final one
    assert all(n.startswith("root/group_normalization") and n.rsplit("/", 1)[1] in ("beta", "gamma") for n in norm_names)
    assert "root/group_normalization/gamma" in names and "root/group_normalization_6/beta" in names
    assert not list(m.buffers())
    step = TrainStep(m, optimizer="momentum", lr=0.05)
    loss = float(step(torch.randn(4, 32, 32, 3), torch.randint(0, 10, (4,))))
    assert loss == loss and abs(loss) < 1e3
    with pytest.raises(ValueError):
        nets_factory.build("cifar10_resnet_v2", 10, resnet_size=8, norm="group")  # 16 channels, 32 groups


def test_buffer_free_model_through_saver_and_buffer_sync(tmp_path):
    from distributed_tensorflow_models_amd import evaluator
    from distributed_tensorflow_models_amd.ckpt.saver import Saver, model_variables
    from distributed_tensorflow_models_amd.parallel.bsp import BufferSync
    kw = dict(resnet_size=8, norm="group", norm_groups=8)
    torch.manual_seed(0)
    a = nets_factory.build("cifar10_resnet_v2", 10, **kw)
    for p in a.parameters():  # betas and gammas away from their constant initial values
        p.data.add_(torch.randn_like(p) * 0.1)
    b = nets_factory.build("cifar10_resnet_v2", 10, **kw)
    path = Saver(model_variables(a)).save(str(tmp_path / "model.ckpt"), global_step=3)
    evaluator.restore_for_eval(b, path, False)
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
    sync = BufferSync(list(a.buffers()), force_comm=True)  # no statistics: every call is a no-op
    sync.issue()
    sync.finish()


def test_default_build_is_the_batch_norm_model():
    for name, kw in (("cifar10_resnet_v2", dict(resnet_size=8)), ("imagenet_resnet_v2", dict(resnet_size=18))):
        default = [n for n, _, _, _ in tf_variables(nets_factory.build(name, 10, **kw))]
        batch = [n for n, _, _, _ in tf_variables(nets_factory.build(name, 10, norm="batch", **kw))]
        assert default == batch and any("moving_mean" in n for n in default)


def test_norm_flag_needs_a_model_that_takes_it():
    assert trainer.norm_model_kw(trainer.PRESETS["resnet"]["model"], "group", 8) == dict(norm="group", norm_groups=8)
    assert trainer.norm_model_kw(trainer.PRESETS["vgg"]["model"], "batch", 32) == {}
    with pytest.raises(ValueError):
        trainer.norm_model_kw(trainer.PRESETS["vgg"]["model"], "group", 32)
    with pytest.raises(ValueError):
        trainer.norm_model_kw(trainer.PRESETS["resnet"]["model"], "layer", 32)
