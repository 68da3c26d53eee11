"""The one input stage of the frame-wise layers (esmdiff_amd/pairs.py: atoms, given_mask, _frames) on the host: no device is needed
for what is checked here."""
import numpy as np
import pytest
import torch

from esmdiff_amd import accessibility, pairs, secondary, torsions


def test_atoms_is_what_the_three_layers_call():
    rng = np.random.default_rng(0)
    x3, x4, ca = rng.normal(size=(2, 7, 3, 3)), rng.normal(size=(2, 7, 4, 3)), rng.normal(size=(5, 7, 3))
    assert torsions.backbone_array(x3).shape == (2, 7, 3, 3) and torsions.backbone_array(x4[0]).shape == (1, 7, 4, 3)
    with_o = secondary.backbone_array(torch.as_tensor(x3, dtype=torch.float32))
    assert with_o.shape == (2, 7, 4, 3) and with_o.dtype == np.float64 and with_o.flags.c_contiguous
    assert np.array_equal(with_o[:, :, 3], secondary.infer_oxygen(with_o[:, :, :3]), equal_nan=True) and np.isnan(with_o[:, -1, 3]).all()
    assert np.array_equal(accessibility.atom_array(x3), secondary.backbone_array(x3), equal_nan=True)
    assert accessibility.atom_array(ca).shape == (5, 7, 1, 3)             # a middle axis that is no atom count: CA traces
    assert accessibility.atom_array(x4[0]).shape == (1, 7, 4, 3)          # (L, 4, 3): one frame
    for fn, text in ((secondary.backbone_array, "backbones should be"), (torsions.backbone_array, "backbones should be"),
                     (accessibility.atom_array, "atoms should be")):
        with pytest.raises(AssertionError, match=text + ".*got \\(2, 7, 2, 3\\)"):
            fn(np.zeros((2, 7, 2, 3)))
    with pytest.raises(AssertionError, match="got \\(1, 5, 7, 3\\)"):
        torsions.backbone_array(ca)                                       # no CA traces where torsions are asked for


def test_given_mask_without_holes_needs_no_device():
    given, mk = pairs.given_mask(None, 3, 4)
    assert given.dtype == bool and given.shape == (3, 4) and given.all() and mk is None
    given, mk = pairs.given_mask(torch.ones(4, dtype=torch.uint8), 3, 4)      # (L,) is every frame's
    assert given.shape == (3, 4) and given.all() and given.flags.writeable and mk is None


def test_frames_states_the_shape_it_wants():
    X = torch.zeros((2, 5, 3, 3), dtype=torch.float64)
    assert pairs._frames(X, None, ((3, 4), 3)) == (2, 5) and pairs._frames(X, torch.ones((2, 5), dtype=torch.uint8), (None, 3)) == (2, 5)
    with pytest.raises(AssertionError, match="f64 \\(n, L, 4, 3\\) frames, got torch.float64 \\(2, 5, 3, 3\\)"):
        pairs._frames(X, None, (4, 3))
    with pytest.raises(AssertionError, match="f64 \\(n, L, 3 or 4, 3\\) frames, got torch.float32"):
        pairs._frames(X.float(), None, ((3, 4), 3))
    with pytest.raises(AssertionError, match="f64 \\(n, L, 3\\) frames"):
        pairs._frames(X, None, (3,))
    with pytest.raises(AssertionError, match="the mask is u8"):
        pairs._frames(X, torch.ones((2, 5), dtype=torch.bool), (None, 3))
