"""`upstream.tmssq_stft` past the 65535 grid-dimension limit: a batch of 65537 signals runs the operator
and the scatter in two launches and the walk, whose grid folds batch x rows, in ten; the first and the last signal equal
their single calls."""
import numpy as np
import pytest

from ssqueeze_rs_amd import upstream as up
from tests.test_gpu_tsst import two_chirps, window

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])
def test_a_batch_of_65537_signals(rdt):
    base = np.stack([two_chirps(16, 70 + b) for b in range(7)]).astype(rdt)
    base[:, 5] += 4.0                                         # an impulse: targets that move
    idx = np.arange(65537) % 7
    kw = dict(n_fft=16, n_iter=2, get_tau=True, get_targets=True)
    win = window(16)
    Tx, Sx, _, _, tau, tgt = up.tmssq_stft(np.ascontiguousarray(base[idx]), win, **kw)
    assert Tx.shape == (65537, 9, 16)
    for b in (0, 65534, 65535, 65536):
        one = up.tmssq_stft(base[idx[b]], win, **kw)
        assert one[0].any() and (one[5] != np.arange(16)).any()
        for got, want in zip((Tx[b], Sx[b], tau[b], tgt[b]), (one[0], one[1], one[4], one[5])):
            assert np.array_equal(got, want), b
    Tb = up.tmssq_stft(base, win, **kw)
    assert np.array_equal(Tx, Tb[0][idx]) and np.array_equal(tgt, Tb[5][idx])
