"""AnomalyDetector (reference: recnn/nn/models.py:7-38) and Plotter.kde_reconstruction_error (recnn/utils/plot.py:96-122):
the parts that need no GPU -- names, state_dict layout, seeded construction, weight loading, the loud no-GPU failure, and the
figure built from any detector's rec_error."""
import numpy as np
import pytest
import torch
import torch.nn as nn

REF_KEYS = [
    ("ae.0.weight", (64, 128)), ("ae.0.bias", (64,)),
    ("ae.2.weight", (64,)), ("ae.2.bias", (64,)), ("ae.2.running_mean", (64,)), ("ae.2.running_var", (64,)),
    ("ae.2.num_batches_tracked", ()),
    ("ae.3.weight", (32, 64)), ("ae.3.bias", (32,)),
    ("ae.5.weight", (32,)), ("ae.5.bias", (32,)), ("ae.5.running_mean", (32,)), ("ae.5.running_var", (32,)),
    ("ae.5.num_batches_tracked", ()),
    ("ae.6.weight", (64, 32)), ("ae.6.bias", (64,)),
    ("ae.8.weight", (64,)), ("ae.8.bias", (64,)), ("ae.8.running_mean", (64,)), ("ae.8.running_var", (64,)),
    ("ae.8.num_batches_tracked", ()),
    ("ae.9.weight", (128, 64)), ("ae.9.bias", (128,)),
]


def _reference_sequential():
    return nn.Sequential(nn.Linear(128, 64), nn.ReLU(), nn.BatchNorm1d(64), nn.Linear(64, 32), nn.ReLU(), nn.BatchNorm1d(32),
                         nn.Linear(32, 64), nn.ReLU(), nn.BatchNorm1d(64), nn.Linear(64, 128), nn.ReLU())


def test_names_resolve():
    import recnn
    from recnn.nn.models import AnomalyDetector
    assert recnn.nn.AnomalyDetector is AnomalyDetector
    assert "AnomalyDetector" in recnn.nn.models.__all__


def test_state_dict_layout_matches_reference():
    from recnn.nn.models import AnomalyDetector
    sd = AnomalyDetector().state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == REF_KEYS


def test_seeded_construction_equals_reference_sequential():
    from recnn.nn.models import AnomalyDetector
    torch.manual_seed(123)
    ref = _reference_sequential()
    torch.manual_seed(123)
    ad = AnomalyDetector()
    for (k, v), (k2, v2) in zip(ad.ae.state_dict().items(), ref.state_dict().items()):
        assert k == k2 and torch.equal(v, v2), k
    after_ad = torch.rand(3)                 # the generator is left where the reference construction leaves it
    torch.manual_seed(123)
    _reference_sequential()
    assert torch.equal(after_ad, torch.rand(3))


def test_load_state_dict_of_reference_keys():
    from recnn.nn.models import AnomalyDetector
    torch.manual_seed(1)
    src = {("ae." + k): v.clone() for k, v in _reference_sequential().state_dict().items()}
    src["ae.5.running_var"] = torch.full((32,), 2.5)
    ad = AnomalyDetector()
    ad.load_state_dict(src)
    for k, v in ad.state_dict().items():
        assert torch.equal(v, src[k]), k


def test_unsupported_batchnorm_settings_raise():
    from recnn.nn.models import AnomalyDetector
    from recnn_amd.nn import functional as F
    for attr, val in (("momentum", None), ("affine", False), ("track_running_stats", False)):
        ad = AnomalyDetector()
        setattr(ad.ae[5], attr, val)
        with pytest.raises(NotImplementedError):
            F._ae_layers(ad.ae)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_gpu_means_loud_failure_not_fallback():
    from recnn.nn.models import AnomalyDetector
    from recnn_amd import _lib as L
    ad = AnomalyDetector()
    x = torch.rand(8, 128)
    for mode in (ad.train, ad.eval):
        mode()
        with pytest.raises(L.RecnnHipError):
            ad(x)
        with pytest.raises(L.RecnnHipError):
            ad.rec_error(x)


class _DuckDetector:
    """rec_error = squared row norm * 100 (any detector with a rec_error method will do)"""

    def rec_error(self, x):
        return (x ** 2).sum(1) * 100.0


def test_kde_reconstruction_error_figure():
    from recnn_amd.utils.plot import Plotter
    rng = np.random.default_rng(0)
    true_actions = rng.random((300, 128)).astype(np.float32)
    gen_actions = torch.as_tensor(rng.random((50, 128)).astype(np.float32) * 1.5)
    fig = Plotter.kde_reconstruction_error(_DuckDetector(), gen_actions, true_actions)
    ax = fig.axes[0]
    lines = ax.get_lines()
    assert [ln.get_label() for ln in lines] == ["true dist", "generated dist"]
    assert [ln.get_color() for ln in lines] == ["b", "r"]
    for ln in lines:
        xs = ln.get_xdata()
        assert len(xs) == 100 and xs[0] == 0 and xs[-1] == 1000
    assert ax.get_legend() is not None
    assert tuple(fig.get_size_inches()) == (16, 10)
