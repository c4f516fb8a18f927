"""`padsignal` of the vendored upstream (old/ssqueezepy/utils/common.py:108-158) restated with np.pad for all five pad
types, with the oracle's signature and return: `(xp, n_up, n1, n2)`.

The oracle (oracle/upstream_oracle.py) restates 'reflect' and 'zero' only; the GPU tests of the other modes patch its
`padsignal` with this one.  'symmetric' is np.pad's: upstream slices it out of one reversed copy (common.py:144-149),
which is the same thing while a pad is no wider than the signal and comes up short beyond that."""
import numpy as np

NP_MODE = {"zero": "constant", "reflect": "reflect", "symmetric": "symmetric", "replicate": "edge", "wrap": "wrap"}


def p2up(n):                                             # common.py:32-51
    up = int(2 ** (1 + np.round(np.log2(n))))
    n2 = int((up - n) // 2)
    n1 = int(up - n - n2)
    return up, n1, n2


def padsignal(x, padtype="reflect", padlength=None):
    if padtype not in NP_MODE:
        raise ValueError(f"padtype {padtype!r}: one of {sorted(NP_MODE)}")
    x = np.asarray(x)
    N = x.shape[-1]
    if padlength is None:
        n_up, n1, n2 = p2up(N)
    else:                                                # common.py:114-120: the larger half on the left
        n_up = int(padlength)
        n2 = (n_up - N) // 2
        n1 = n_up - N - n2
    width = (n1, n2) if x.ndim == 1 else [(0, 0), (n1, n2)]
    return np.pad(x, width, mode=NP_MODE[padtype]), n_up, n1, n2
