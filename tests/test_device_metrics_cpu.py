"""The device_metrics switch and ops.auc_sorted, as far as they go without a GPU."""
import numpy as np
import pytest
import torch

from test_regression_cpu import cpu_model


def model():
    m = cpu_model(["binary", "binary"])
    return m, m.config


def test_switch_is_off_when_the_key_is_absent():
    m, cfg = model()
    assert "device_metrics" not in cfg["optim_config"]
    assert m.device_metrics is False
    m.compile("adam", ["binary_crossentropy"] * 2, ["auc"])
    assert m.device_metrics is False


def test_switch_parses_from_config_compile_and_attribute():
    m, cfg = model()
    for v, want in ((True, True), (False, False), (1, True), (0, False), ("true", True), ("false", False)):
        cfg2 = {k: dict(d) for k, d in cfg.items()}
        cfg2["optim_config"]["device_metrics"] = v
        assert type(m)(m.dnn_feature_columns, config=cfg2).device_metrics is want, v
    with pytest.raises(ValueError):
        cfg2["optim_config"]["device_metrics"] = "perhaps"
        type(m)(m.dnn_feature_columns, config=cfg2)
    m.compile("adam", ["binary_crossentropy"] * 2, ["auc"], device_metrics=True)
    assert m.device_metrics is True
    m.compile("adam", ["binary_crossentropy"] * 2, ["auc"])  # None: left as it is
    assert m.device_metrics is True
    m.compile("adam", ["binary_crossentropy"] * 2, ["auc"], device_metrics=False)
    assert m.device_metrics is False
    m.device_metrics = True
    assert m.device_metrics is True


def test_auc_sorted_refuses_cpu_tensors():
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import ops
    from mmlrec_amd._lib import MMLError
    p = torch.rand(100, 2)
    with pytest.raises(MMLError):
        ops.auc_sorted(p, (p > 0.5).float())
    with pytest.raises(MMLError):
        ops.auc_sorted(p, (p > 0.5).float(), seg=10, mask=torch.ones(100, 1), return_counts=True)


def test_key_image_is_monotone():
    """a < b <=> image(a) < image(b), a == b <=> equal images, on a sorted sample with both zeros, denormals, the largest
    finite values and the neighbours of 0 and 1."""
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd.ops import auc_key_image
    rng = np.random.default_rng(0)
    fmax, tiny = np.finfo(np.float32).max, np.float32(1e-45)
    special = np.array([-fmax, -1.0, -tiny, -0.0, 0.0, tiny, 2 * tiny, np.finfo(np.float32).tiny, 0.5,
                        np.nextafter(np.float32(1), np.float32(0)), 1.0, np.nextafter(np.float32(1), np.float32(2)), fmax],
                       np.float32)
    sample = np.concatenate([special, rng.standard_normal(500).astype(np.float32),
                             (rng.standard_normal(200) * 1e-40).astype(np.float32)])
    sample = np.sort(sample, kind="stable")
    img = [auc_key_image(v) for v in sample]
    assert all(0 <= i < 1 << 32 for i in img)
    for a, b, ia, ib in zip(sample[:-1], sample[1:], img[:-1], img[1:]):
        assert (a < b) == (ia < ib) and (a == b) == (ia == ib), (a, b, ia, ib)
    assert auc_key_image(-0.0) == auc_key_image(0.0) == 0x80000000
    # every finite image lies below the image of +inf, and the mask sentinel above everything
    assert max(img) < auc_key_image(float("inf")) < 0xffffffff
    assert auc_key_image(-float("inf")) < min(img)
