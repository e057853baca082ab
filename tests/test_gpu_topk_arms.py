"""GPU parity: every arm of topk_kernel (csrc/topk.h) through hipts_topk against the CPU oracle -- ids equal, values bit-equal.
The rows come from tests/topk_arms.py; test_topk_arms_host.py holds each case to the arm it is named for."""
import numpy as np
import pytest

import topk_arms

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(topk_arms.CASES))
def test_topk_arm(name):
    import torch
    from hiptagsearch import _lib
    from oracle import search as osearch
    _, n, k, _ = topk_arms.CASES[name]
    vals = topk_arms.rows(name)
    nq = len(vals)
    dev = torch.from_numpy(vals).cuda()
    ids = np.empty((nq, k), np.int32)
    out = np.empty((nq, k), np.float64)
    _lib.call("hipts_topk", _lib.ptr(dev), nq, _lib.c_int64(n), k, _lib.ptr(ids), _lib.ptr(out), _lib.HOST, 0, None)
    for r in range(nq):
        wi, wv = osearch.topk(vals[r], k)
        np.testing.assert_array_equal(ids[r], wi, err_msg="%s row %d" % (name, r))
        assert out[r].tobytes() == wv.tobytes(), (name, r)
