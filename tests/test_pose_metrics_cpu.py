"""CPU (no GPU): utils.ply_loader.load_ply on ASCII and binary files, the lazy re-exports of utils/__init__.py, and the
host-side re / te / depth_im_to_dist_im against the reference's values (tests/golden/pose_metrics.npz)."""
import os
import struct
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "pose_metrics.npz"))
PTS = np.array([[0.0, 0.0, 0.0], [1.5, 0.0, 0.25], [0.0, 2.0, -1.0], [1.0, 1.0, 1.0]])
NRM = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.6, 0.8, 0.0]])
COL = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 20, 30]])
FACES = np.array([[0, 1, 2], [1, 3, 2]])


def write_ply(path, binary):
    head = ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii"), "comment test mesh",
            "element vertex %d" % len(PTS), "property float x", "property float y", "property float z", "property float nx",
            "property float ny", "property float nz", "property uchar red", "property uchar green", "property uchar blue",
            "element face %d" % len(FACES), "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode())
        for p, n, c in zip(PTS, NRM, COL):
            if binary:
                f.write(struct.pack("<6f3B", *p, *n, *c))
            else:
                f.write(("%g %g %g %g %g %g %d %d %d\n" % (*p, *n, *c)).encode())
        for tri in FACES:
            f.write(struct.pack("<B3i", 3, *tri) if binary else ("3 %d %d %d\n" % tuple(tri)).encode())


def test_load_ply_ascii_and_binary(tmp_path):
    from pyrapose_amd.utils.ply_loader import load_ply
    for binary in (False, True):
        path = str(tmp_path / ("m_%d.ply" % binary))
        write_ply(path, binary)
        m = load_ply(path)
        assert set(m) == {"pts", "faces", "normals", "colors"}
        for k, want in (("pts", PTS), ("faces", FACES), ("normals", NRM), ("colors", COL)):
            assert m[k].dtype == np.float64 and m[k].shape == want.shape
            np.testing.assert_allclose(m[k], want, rtol=1e-7, atol=1e-7)


def test_load_ply_rejects_quads(tmp_path):
    import pytest
    from pyrapose_amd.utils.ply_loader import load_ply
    path = str(tmp_path / "quad.ply")
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
                "element face 1\nproperty list uchar int vertex_indices\nend_header\n0 0 0\n1 0 0\n1 1 0\n0 1 0\n4 0 1 2 3\n")
    with pytest.raises(ValueError):
        load_ply(path)


def test_utils_exports_are_lazy():
    code = ("import sys\nimport pyrapose_amd.utils, pyrapose_amd.utils.ply_loader\n"
            "assert 'pyrapose_amd._lib' not in sys.modules, 'the library loaded on import'\n"
            "from pyrapose_amd.utils import reproj, add, adi, re, te\n"
            "assert 'pyrapose_amd._lib' in sys.modules\n"
            "import pyrapose_amd.utils.pose_error as PE\n"
            "assert (reproj, add, adi, re, te) == (PE.reproj, PE.add, PE.adi, PE.re, PE.te)\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    import pyrapose_amd.utils as U
    import pytest
    with pytest.raises(AttributeError):
        U.no_such_name


def test_re_te_and_dist_im_match_reference_on_the_host():
    from pyrapose_amd.utils import pose_error as PE
    g = lambda k: G["rt_" + k]
    assert PE.re_batch(g("R_est"), g("R_gt")).tolist() == g("re").tolist()
    assert PE.te_batch(g("t_est"), g("t_gt")).tolist() == g("te").tolist()
    assert PE.re(g("R_gt")[0], g("R_gt")[0]) == 0.0
    d = PE.depth_im_to_dist_im(G["v0_depth_test"][0], G["v0_K"])
    assert d.shape == G["v0_depth_test"][0].shape and np.array_equal(d > 0, G["v0_depth_test"][0] > 0)
