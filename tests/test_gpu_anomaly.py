"""AnomalyDetector on the GPU (csrc/anomaly.hip) against torch's own modules on the CPU in float64."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu


def _detector(seed=0):
    """A detector with non-trivial BatchNorm state (gamma, beta, running statistics away from their defaults), on the GPU."""
    from recnn.nn.models import AnomalyDetector
    torch.manual_seed(seed)
    ad = AnomalyDetector()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for i in (2, 5, 8):
            bn = ad.ae[i]
            c = bn.num_features
            bn.weight.copy_(0.5 + torch.rand(c, generator=g))
            bn.bias.copy_(0.3 * torch.randn(c, generator=g))
            bn.running_mean.copy_(0.2 + 0.3 * torch.rand(c, generator=g))
            bn.running_var.copy_(0.05 + 0.3 * torch.rand(c, generator=g))
            bn.num_batches_tracked.fill_(7)
    return ad.cuda()


def _x(rows, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(rows, 128, generator=g)


def _ref(ad):
    return copy.deepcopy(ad).cpu().double()


def _close(got, ref, tol, what=""):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    assert err <= tol * max(scale, 1e-30), f"{what}: max|d| {err:.3e} vs {tol:.0e} * {scale:.3e}"


@pytest.mark.parametrize("rows", [1, 2, 63, 64, 65, 1000, 27278])
def test_eval_forward_and_rec_error(cuda, rows):
    ad = _detector().eval()
    ref = _ref(ad).eval()
    x = _x(rows)
    with torch.no_grad():
        out_ref = ref.ae(x.double())
        err_ref = ((x.double() - out_ref) ** 2).sum(1)
        out = ad(x.cuda())
        err = ad.rec_error(x.cuda())
    _close(out, out_ref, 2e-5, "forward")
    _close(err, err_ref, 2e-5, "rec_error")
    assert out.dtype == torch.float32 and err.shape == (rows,)


def test_eval_strided_rows_and_empty(cuda):
    ad = _detector().eval()
    ref = _ref(ad).eval()
    big = _x(600).cuda()
    x = big.view(300, 256)[:, 64:192]                     # a row view with ld 256 and a 64-float offset
    assert x.stride() == (256, 1)
    with torch.no_grad():
        out_ref = ref.ae(x.cpu().double())
        _close(ad(x), out_ref, 2e-5, "strided forward")
        _close(ad.rec_error(x), ((x.cpu().double() - out_ref) ** 2).sum(1), 2e-5, "strided rec_error")
        odd = big[1:, :].reshape(-1)[3:3 + 128 * 50].view(50, 128)   # not 16-byte aligned
        _close(ad(odd), ref.ae(odd.cpu().double()), 2e-5, "misaligned forward")
        e = torch.empty(0, 128, device=cuda)
        assert ad(e).shape == (0, 128) and ad.rec_error(e).shape == (0,)


@pytest.mark.parametrize("rows", [2, 100, 15000])
def test_train_forward_updates_running_stats(cuda, rows):
    ad = _detector().train()
    ref = _ref(ad).train()
    x = _x(rows, seed=rows)
    with torch.no_grad():
        out = ad(x.cuda())
        out_ref = ref.ae(x.double())
    _close(out, out_ref, 2e-5, "train forward")
    for i in (2, 5, 8):
        _close(ad.ae[i].running_mean, ref.ae[i].running_mean, 2e-5, f"running_mean {i}")
        _close(ad.ae[i].running_var, ref.ae[i].running_var, 2e-5, f"running_var {i}")
        assert int(ad.ae[i].num_batches_tracked) == 8
    # a train-mode rec_error updates them too (what the training notebook calls)
    err = ad.rec_error(x.cuda())
    with torch.no_grad():
        err_ref = ((x.double() - ref.ae(x.double())) ** 2).sum(1)
    _close(err, err_ref, 2e-5, "train rec_error")
    _close(ad.ae[8].running_var, ref.ae[8].running_var, 2e-5, "running_var after rec_error")
    assert int(ad.ae[2].num_batches_tracked) == 9


def test_train_one_row_raises(cuda):
    ad = _detector().train()
    with pytest.raises(ValueError):
        ad(torch.rand(1, 128, device=cuda))


def _grads(model, x, xgrad):
    x = x.clone().requires_grad_(xgrad)
    out = model.ae(x) if x.device.type == "cpu" else model(x)      # the fp64 oracle runs torch's own modules
    loss = nn.MSELoss()(out, x)
    loss.backward()
    params = [p.grad for p in model.parameters()]
    return loss, params, (x.grad if xgrad else None)


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("rows", [100, 4096])
def test_gradients(cuda, train, rows):
    ad = _detector()
    ref = _ref(ad)
    ad.train(train)
    ref.train(train)
    x = _x(rows, seed=11)
    loss, g, gx = _grads(ad, x.cuda(), True)
    loss_ref, g_ref, gx_ref = _grads(ref, x.double(), True)
    assert len(g) == 14
    names = [n for n, _ in ad.named_parameters()]
    for n, a, b in zip(names, g, g_ref):
        _close(a, b, 1e-4, n)
    _close(gx, gx_ref, 1e-4, "x")
    assert abs(loss.item() - loss_ref.item()) <= 1e-5 * abs(loss_ref.item())
    # without x.requires_grad: no dx, the same parameter gradients
    ad.zero_grad()
    _, g2, gx2 = _grads(ad, x.cuda(), False)
    assert gx2 is None
    if not train:
        for a, b in zip(g, g2):
            assert torch.equal(a, b)


def test_determinism(cuda):
    runs = []
    for _ in range(2):
        ad = _detector().train()
        x = _x(5000, seed=5).cuda()
        _, g, gx = _grads(ad, x, True)
        stats = [getattr(ad.ae[i], k).clone() for i in (2, 5, 8) for k in ("running_mean", "running_var")]
        with torch.no_grad():
            out = ad(x)
        ad.eval()
        runs.append([out, ad.rec_error(x), gx] + g + stats)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_weight_reload_changes_result(cuda):
    ad = _detector().eval()
    x = _x(256).cuda()
    with torch.no_grad():
        before = ad(x).clone()
        err_before = ad.rec_error(x).clone()
        other = _detector(seed=9)
        ad.load_state_dict(other.state_dict())
        after = ad(x)
        _close(after, _ref(ad).eval().ae(x.cpu().double()), 2e-5, "after reload")
    assert not torch.equal(before, after)
    assert not torch.equal(err_before, ad.rec_error(x))


def test_training_curve_matches_fp64(cuda):
    from recnn_amd.optim import Adam
    ad = _detector(seed=4).train()
    ref = _ref(ad).train()
    opt = Adam(ad.parameters(), lr=1e-3)
    opt_ref = torch.optim.Adam(ref.parameters(), lr=1e-3)
    crit = nn.MSELoss()
    g = torch.Generator().manual_seed(17)
    base = torch.rand(4096, 128, generator=g)
    for step in range(20):
        x = base[torch.randperm(4096, generator=g)]
        opt.zero_grad()
        loss = crit(ad(x.cuda()), x.cuda())
        loss.backward()
        opt.step()
        opt_ref.zero_grad()
        xd = x.double()
        loss_ref = crit(ref.ae(xd), xd)
        loss_ref.backward()
        opt_ref.step()
        assert abs(float(loss) - float(loss_ref)) <= 1e-4 * abs(float(loss_ref)), (step, float(loss), float(loss_ref))


def test_no_eager_torch_on_the_detector_path(cuda):
    ad = _detector()
    x = _x(2048).cuda()
    for mode in (ad.eval, ad.train):
        mode()
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
            with torch.no_grad():
                ad(x)
                ad.rec_error(x)
            ad(x).sum()
        names = {e.name for e in prof.events()}
        bad = [n for n in names if n in ("aten::addmm", "aten::linear") or ("batch_norm" in n and n.startswith("aten::"))]
        assert not bad, bad


def test_notebook_kde_call(cuda):
    from recnn_amd.utils.plot import Plotter
    ad = _detector().eval()
    catalogue = np.random.default_rng(0).random((3000, 128)).astype(np.float32)
    gen = torch.rand(200, 128, device=cuda)
    fig = Plotter.kde_reconstruction_error(ad, gen, catalogue, cuda)
    assert [ln.get_label() for ln in fig.axes[0].get_lines()] == ["true dist", "generated dist"]
