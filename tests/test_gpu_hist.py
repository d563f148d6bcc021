"""FeatureHistogram on the GPU (sa_hist_codes / _build / _finish): the device
form equals the host form bit for bit in the codes, the float64 array and the
nested form; one case goes straight against the fsum reference."""
import numpy as np
import pytest
from gpu_copies import _dev, _host
from hist_cases import assert_within_bound, fsum_reference, make_case

pytestmark = pytest.mark.gpu

from sfl_amd import kernels as K  # noqa: E402
from sfl_amd.ml.boost import FeatureHistogram  # noqa: E402

SLOTS_255 = K.hist_geometry(255, 64, 5)[1]  # slots per launch at Bmax = 255


def _both(x, splits, grad, hess, node, n_nodes, valid=None, use_missing=True, misalign=False, codes=None):
    """Host and device forms of one batch; asserts equal bits; returns the
    device object, the host array and its nested form."""
    import torch

    host, dev = FeatureHistogram(splits, use_missing), FeatureHistogram(splits, use_missing)
    hc = host.bind(x) if codes is None else codes
    dc = dev.bind(_dev(x, misalign).view(x.shape)) if codes is None else _dev(codes).view(codes.shape)
    assert dc.is_cuda and dc.dtype == torch.uint8 and np.array_equal(_host(dc), hc)
    host.set_gradients(grad, hess)
    dev.set_gradients(_dev(grad, misalign), _dev(hess, misalign))
    assert (host.last_report["k_grad"], host.last_report["k_hess"]) == (dev.last_report["k_grad"],
                                                                        dev.last_report["k_hess"])
    want, want_lists = host.calculate_histogram(hc, node, n_nodes, valid, as_lists=True)
    got, got_lists = dev.calculate_histogram(dc, _dev(node), n_nodes, valid, as_lists=True)
    assert got.is_cuda and got.dtype == torch.float64
    assert np.array_equal(_host(got).view(np.uint64), want.view(np.uint64))
    for a, b in zip(sum(got_lists, []), sum(want_lists, [])):
        assert np.array_equal(a, b) and np.shape(a) == np.shape(b)
    return dev, dc, want, want_lists


CASES = [(rows, 5, 33, 2, "f4", "f4") for rows in (1, 255, 256, 257, 1023, 4100, 70003)] \
    + [(1023, f, 33, 2, "f4", "f4") for f in (1, 3, 4, 33)] \
    + [(1023, 5, b, 2, "f4", "f4") for b in (1, 2, 255)] \
    + [(1023, 4, 255, n, "f4", "f4") for n in (1, 20, SLOTS_255 + 1)] \
    + [(1023, 5, 33, 2, "f8", "f4"), (1023, 5, 33, 2, "f4", "f8"), (1023, 8, 33, 20, "f8", "f8")]


@pytest.mark.parametrize("rows,nf,bmax,n_nodes,xt,gt", CASES)
def test_device_form_equals_host_form(rows, nf, bmax, n_nodes, xt, gt):
    x, splits, grad, hess, node = make_case(rows, nf, bmax, n_nodes, np.dtype(xt), np.dtype(gt))
    valid = {f: f != 1 for f in range(nf)} if nf > 2 else None
    dev, *_ = _both(x, splits, grad, hess, node, n_nodes, valid, use_missing=rows % 2 == 1)
    assert dev.last_report["slot_chunks"] == K.hist_geometry(bmax, n_nodes, nf)[2]
    assert dev.last_report["host_fallback"] == 0


@pytest.mark.parametrize("xt,gt", [("f4", "f4"), ("f8", "f8")])
def test_views_offset_by_one_element(xt, gt):
    x, splits, grad, hess, node = make_case(4100, 5, 33, 2, np.dtype(xt), np.dtype(gt))
    _both(x, splits, grad, hess, node, 2, misalign=True)


def test_against_the_fsum_reference_with_the_cancelling_gradients():
    """257 float32 gradients with 1e8, -1e8, 1: the device result itself is
    within N 2^-(k + 1) of the exact sums, where a float32 sum is off by ~7."""
    x, splits, grad, hess, node = make_case(257, 3, 33, 2)
    grad[:3] = [1e8, -1e8, 1]
    node[:3] = 0
    dev, dc, _, _ = _both(x, splits, grad, hess, node, 2)
    got = dev.as_lists(dev.calculate_histogram(dc, _dev(node), 2))
    assert_within_bound(got, fsum_reference(x, splits, grad, hess, node, 2, [True] * 3, True),
                        dev.last_report["k_grad"], dev.last_report["k_hess"])


@pytest.mark.parametrize("at", [0, 3, 4, 255, 256, 1021, 1022])
def test_one_decisive_row(at):
    """Every row beyond the last split point but one, whose code is 0: each
    bucket holds exactly that row's gradient."""
    rows = 1023
    x = np.full((rows, 4), 9.0, dtype=np.float32)
    x[at] = -9.0
    grad = np.arange(1, rows + 1, dtype=np.float32)
    _, _, want, _ = _both(x, [np.linspace(-1, 1, 7)] * 4, grad, grad, np.zeros(rows, np.int32), 1)
    assert (want[0, :, :7, 0] == at + 1).all() and (want[0, :, :7, 2] == 1).all() and (want[0, :, 7, 2] == rows - 1).all()


def test_conflicts_empty_slots_big_sums_and_dirty_scratch():
    import torch

    rows = 4100
    x = np.zeros((rows, 4), dtype=np.float32)
    splits = [np.array([1.0, 2.0])] * 4
    grad = np.full(rows, 0.75, dtype=np.float64)
    grad[0] = 2.0 ** -49  # the sum of q passes 2^53 with low bits set: the conversion to float64 rounds
    # every row in one bin of one node: the worst atomic conflict
    dev, dc, want, _ = _both(x, splits, grad, grad, np.ones(rows, np.int32), 2)
    k = dev.last_report["k_grad"]
    assert int(np.rint(np.ldexp(grad, k)).astype(np.int64).sum()) > 2 ** 53 and not want[0].any()
    # the same bits twice over scratch filled with 0xFF
    node = _dev(np.ones(rows, np.int32))
    for _ in range(2):
        dev._dev[dc.device]["scratch"].fill_(0xFF)
        again = dev.calculate_histogram(dc, node, 2)
        assert np.array_equal(_host(again).view(np.uint64), want.view(np.uint64))
    # every row at slot -1: all zeros
    none = dev.calculate_histogram(dc, _dev(np.full(rows, -1, np.int32)), 2)
    assert not _host(none).any() and none.dtype == torch.float64
