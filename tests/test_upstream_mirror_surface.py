"""The upstream mirror's higher-order GMW surface, decided before the GPU is touched: `cwt_higher_order`'s signature
(old/ssqueezepy/_cwt.py:515) and the order options that raise ValueError -- a bare int `order` other than 0 on `cwt`
(as before; `order=(k,)` or `cwt_higher_order` computes it), orders with a Morlet wavelet, negative orders, orders above
the built maximum, and higher orders with `l1_norm=False` (upstream's energy-normalised GMW is not built)."""
import inspect

import numpy as np
import pytest


def test_cwt_higher_order_signature():
    from ssqueeze_rs_amd import upstream as up
    params = list(inspect.signature(up.cwt_higher_order).parameters.items())
    assert [(k, v.default) for k, v in params[1:5]] == [("wavelet", "gmw"), ("order", 1), ("average", None),
                                                        ("astensor", True)]
    assert params[5][1].kind is inspect.Parameter.VAR_KEYWORD


def test_order_options_outside_the_subset_raise_before_the_gpu():
    from ssqueeze_rs_amd import upstream as up
    x = np.zeros(64)
    sc = 2.0 ** (np.arange(8, 24) / 8)
    for call in (lambda: up.cwt(x, scales=sc, order=2),
                 lambda: up.cwt(x, scales=sc, order=np.int64(3), average=True),
                 lambda: up.cwt(x, "morlet", scales=sc, order=(0, 1)),
                 lambda: up.cwt(x, scales=sc, order=(1, -1)),
                 lambda: up.cwt(x, scales=sc, order=(up.GMW_MAX_ORDER + 1,)),
                 lambda: up.cwt(x, scales=sc, order=(0, 1), l1_norm=False),
                 lambda: up.cwt(x, ("gmw", {"order": 1}), scales=sc),
                 lambda: up.cwt_higher_order(x, "morlet", order=1, scales=sc),
                 lambda: up.cwt_higher_order(x, order=-1, scales=sc),
                 lambda: up.ssq_cwt(x, "morlet", scales=sc, order=2),
                 lambda: up.ssq_cwt(x, scales=sc, order=-2)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        up.cwt_higher_order(x, order=1, scales=sc, bogus=1)
