"""Tree-model inputs from draw masks, the host side: the cut rule behind ``bit_counts``, the lag-window
specification the GPU tests compare against, and the CLI's configuration errors for ``--data-source device``."""
import os
import subprocess
import sys

import numpy as np
import pytest

from _tree_inputs_spec import lag_rows_spec, random_masks, unpack

from euromillioner_amd.data.draws import DrawSet, mask_bits
from euromillioner_amd.models.forest import draw_features
from euromillioner_amd.models.gbdt import apply_bins, cuts_from_bit_counts, make_cuts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_cuts(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype == np.float64 and np.array_equal(x, y)


def test_cuts_rule_equals_make_cuts():
    g = np.random.default_rng(0)
    X = (g.random((257, 62)) < 0.3).astype(np.float64)
    X[:, 3] = 0.0  # never set
    X[:, 7] = 1.0  # always set
    X[:, 11] = 0.0
    X[5, 11] = 1.0  # set once
    X[:, 12] = 1.0
    X[9, 12] = 0.0  # clear once
    cuts = cuts_from_bit_counts(X.sum(0).astype(np.int64), len(X))
    _same_cuts(cuts, make_cuts(X))
    assert len(cuts[3]) == 0 and len(cuts[7]) == 0 and list(cuts[11]) == [0.5] and list(cuts[12]) == [0.5]
    assert np.array_equal(apply_bins(X, cuts), (X * (np.array([len(c) for c in cuts]) > 0)).astype(np.uint8))


@pytest.mark.parametrize("row", [0, 1])
def test_cuts_rule_single_row(row):
    X = np.zeros((1, 62))
    X[0, ::2] = row
    _same_cuts(cuts_from_bit_counts(X.sum(0).astype(np.int64), 1), make_cuts(X))


@pytest.mark.parametrize("lags", [1, 2, 3, 4])
def test_lag_window_spec_equals_draw_features(lags):
    ds = DrawSet.synthetic(n=300, seed=3, planted=0.5, calendar=False)
    X, Y, F = draw_features(ds.numbers, lags)
    Xs, Ys = lag_rows_spec(mask_bits(ds.numbers), lags, 0, len(ds) - lags)
    assert F == 62 * lags and Xs.shape == (len(ds) - lags, (F + 63) // 64)
    assert np.array_equal(Xs, X) and np.array_equal(Ys, Y)
    a = 17  # a window that starts inside the sequence and ends at the last draw
    Xw, Yw = lag_rows_spec(mask_bits(ds.numbers), lags, a, len(ds) - lags - a)
    assert np.array_equal(Xw, X[a:]) and np.array_equal(Yw, Y[a:])


def test_spec_on_random_masks_drops_the_pad_bits():
    m = random_masks(40, 1)
    assert (m.view(np.uint64) >> np.uint64(62)).any()  # the inputs do carry bits 62-63
    X, Y = lag_rows_spec(m, 4, 0, 36)
    assert not (X[:, 3] >> np.uint64(248 - 192)).any() and not (Y >> np.uint64(62)).any()
    bits = unpack(m)
    assert np.array_equal((X[:, 0] >> np.uint64(62)) & np.uint64(3), (bits[1:37, 0] + 2 * bits[1:37, 1]).astype(np.uint64))


def _cli(args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", "euromillioner_amd"] + args, capture_output=True, text=True,
                       timeout=300, env=env, cwd=ROOT)
    return p.returncode, p.stdout + p.stderr


@pytest.mark.parametrize("model", ["rf", "gbdt"])
def test_cli_device_source_needs_a_gpu(model):
    rc, text = _cli(["train", "--model", model, "--data-source", "device", "--n-draws", "5000", "--device", "cpu"])
    assert rc == 2, text
    assert "needs a GPU" in text


def test_cli_device_source_refuses_the_reference_target():
    rc, text = _cli(["train", "--model", "gbdt", "--data-source", "device", "--n-draws", "5000",
                     "--gbdt-target", "reference"])
    assert rc == 2, text
    assert "gbdt.target=reference" in text and "dates" in text
