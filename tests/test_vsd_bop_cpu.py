"""CPU (no GPU): the numpy restatement of multi-tau VSD (tests/vsd_bop_np.py) in mode 'bop18' against the columns the
reference's own vsd() and visibility masks wrote into tests/golden/pose_metrics.npz -- this pins the restatement before
tests/test_gpu_vsd_bop.py compares the kernel with it -- and what the 'bop19' rule changes."""
import os

import numpy as np

from tests import vsd_bop_np as VN

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_metrics.npz"))


def test_restatement_reproduces_the_reference_columns_in_mode_bop18():
    params = list(zip(G["vsd_cost"], G["vsd_delta"], G["vsd_tau"]))
    assert len(params) == 4 and {str(c) for c, _, _ in params} == {"step", "tlinear"}
    for c in G["vsd_cases"]:
        g = lambda k: G["v%d_%s" % (c, k)]
        dt = g("depth_test")[0] if bool(g("shared")) else g("depth_test")
        for j, (cost, delta, tau) in enumerate(params):
            # the golden tau among others: the column does not depend on its neighbours
            taus = sorted({float(tau), 2.5, 33.0})
            e, inter, uni, vis, px = VN.vsd_multi(dt, g("depth_est"), g("depth_gt"), g("K"), float(delta), taus, str(cost), "bop18")
            col = e[:, taus.index(float(tau))]
            if str(cost) == "step":
                assert np.array_equal(col, g("vsd")[:, j])
            else:
                np.testing.assert_allclose(col, g("vsd")[:, j], rtol=1e-12, atol=0)
            assert np.array_equal(inter, g("inter")[:, j]) and np.array_equal(uni, g("union")[:, j])
            assert np.array_equal(px, (g("depth_gt") > 0).sum(axis=(1, 2))) and (vis <= px).all() and (inter <= vis).all()
            assert (np.diff(e, axis=1) <= 0).all()                        # a larger tolerance never raises the error
    assert (G["v0_union"][5] == 0).all()
    e = VN.vsd_multi(G["v0_depth_test"], G["v0_depth_est"], G["v0_depth_gt"], G["v0_K"], 15.0, [5.0, 20.0], "step", "bop18")[0]
    assert e[5].tolist() == [1.0, 1.0]                                    # the empty union


def test_bop19_counts_rendered_pixels_without_sensor_depth_as_visible():
    g = lambda k: G["v0_" + k]
    dt = g("depth_test").copy()
    rows, cols = np.indices(dt.shape[1:])
    dt[(g("depth_gt") > 0) & ((rows + cols) % 4 == 0)[None]] = 0.0
    taus = [4.5, 9.0, 45.0]
    old = VN.vsd_multi(dt, g("depth_est"), g("depth_gt"), g("K"), 15.0, taus, "step", "bop18")
    new = VN.vsd_multi(dt, g("depth_est"), g("depth_gt"), g("K"), 15.0, taus, "step", "bop19")
    holes = ((g("depth_gt") > 0) & (dt == 0)).sum(axis=(1, 2))
    assert (holes[:5] > 0).all() and holes[5] == 0
    assert np.array_equal(new[3], old[3] + holes)                         # every hole under the render joins visib_gt
    assert np.array_equal(new[4], old[4]) and (new[2] >= old[2]).all() and (new[2][:5] > old[2][:5]).all()
    assert new[0][5].tolist() == [1.0, 1.0, 1.0]
