"""General-inertia arms (full link inertias `mlink`, joint inertias `mjoint`; include/abrk_types.h abrk_arm_inertia):
table format, extractor, normalisation, C ABI layout and loader, and the host build of the row programs against the
reference's own M, g, C (tests/golden/inertia_<arm>.npz, tools/gen_inertia_golden.py).  Runs on CPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from abr_control_amd import _abi, specialize
from tests import compiled_inertia_arms

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
ARMS = compiled_inertia_arms.ARMS


def fixture(arm):
    return compiled_inertia_arms.table(arm), np.load(os.path.join(GOLDEN, f"inertia_{arm}.npz"))


class ChainConfig:
    """a BaseConfig-like SymPy config built from a table the way tools/gen_inertia_golden.py builds the reference's:
    T(link0) = A0, T(joint_i) = T(link_i) AJ[i], T(link_i+1) = T(joint_i) Rz(q_i) B[i], T(EE) = T(link_n) E"""

    def __init__(self, tab):
        import sympy as sp

        n = self.N_JOINTS = int(tab["n_joints"])
        self.N_LINKS = int(tab["n_links_dyn"])
        self.ROBOT_NAME = tab["name"]
        self.START_ANGLES = np.asarray(tab.get("START_ANGLES", np.zeros(n)), dtype=float)
        self.q = [sp.Symbol(f"q{i}") for i in range(n)]
        aff = lambda m: sp.Matrix(np.vstack([np.asarray(m, float), [0, 0, 0, 1]]).tolist())
        self.A0, self.E = aff(tab["A0"]), aff(tab["E"])
        self.AJ, self.B = [aff(m) for m in tab["AJ"]], [aff(m) for m in tab["B"]]
        self._M_LINKS = ([sp.Matrix(m) for m in tab["mlink"]] if "mlink" in tab
                         else [sp.diag(*[float(v) for v in r]) for r in tab["mdiag"]])
        self._M_JOINTS = [sp.Matrix(m) for m in tab["mjoint"]]
        self._sp = sp

    def _calc_T(self, name):
        sp, n = self._sp, self.N_JOINTS
        if name == "link0":
            return self.A0
        if name == "EE":
            return self._calc_T(f"link{n}") * self.E
        if name.startswith("joint"):
            i = int(name[5:])
            return self._calc_T(f"link{i}") * self.AJ[i]
        i = int(name[4:]) - 1
        c, s = sp.cos(self.q[i]), sp.sin(self.q[i])
        return self._calc_T(f"joint{i}") * sp.Matrix([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]) * self.B[i]


def _extract():
    import importlib.util

    spec = importlib.util.spec_from_file_location("extract_arm_table", os.path.join(REPO, "tools", "extract_arm_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.extract


@pytest.mark.parametrize("arm", ARMS)
def test_extractor_reproduces_the_fixture_tables(arm):
    tab, _ = fixture(arm)
    with _quiet():
        got = _extract()(ChainConfig(tab), tab["name"])
    assert sorted(k for k in got if k != "START_ANGLES") == sorted(k for k in tab if k != "START_ANGLES")
    for k in ("n_joints", "n_links_dyn", "has_ee", "name"):
        assert got[k] == tab[k], k
    for k in ("A0", "AJ", "B", "E"):  # static transforms: recovered through a matrix solve
        np.testing.assert_allclose(np.array(got[k], float), np.array(tab[k], float), rtol=0, atol=1e-12, err_msg=k)
    for k in ("mdiag", "mlink", "mjoint"):  # inertias: read as they are
        if k in tab:
            assert np.array_equal(np.array(got[k], float), np.array(tab[k], float)), k
    assert _abi.is_general_inertia(got)


class _quiet:
    def __enter__(self):
        import warnings

        self._w = warnings.catch_warnings()
        self._w.__enter__()
        warnings.simplefilter("ignore")

    def __exit__(self, *a):
        return self._w.__exit__(*a)


def test_extractor_refuses_an_asymmetric_inertia():
    tab, _ = fixture("synthetic4")
    rc = ChainConfig(tab)
    rc._M_JOINTS[2] = rc._M_JOINTS[2].copy()
    rc._M_JOINTS[2][1, 4] += 1e-3
    with _quiet(), pytest.raises(ValueError, match="not symmetric"):
        _extract()(rc, "x")


def test_plain_inertias_normalise_to_the_plain_table():
    tab = _abi.load_table("ur5")
    n = tab["n_joints"]
    t2 = dict(tab, mlink=[np.diag(r).tolist() for r in tab["mdiag"]], mjoint=[np.zeros((6, 6)).tolist()] * n)
    norm = _abi.normalize_table(t2)
    assert "mlink" not in norm and "mjoint" not in norm and not _abi.is_general_inertia(t2)
    assert bytes(_abi.desc_from_table(norm)) == bytes(_abi.desc_from_table(tab))
    assert specialize.arm_key(t2, abi="x") == specialize.arm_key(tab, abi="x")
    assert _abi.render_tab_struct(t2, "Tab_x") == _abi.render_tab_struct(tab, "Tab_x")
    assert bytes(_abi.inertia_from_table(t2)) == bytes(_abi.inertia_from_table(tab))


def test_general_inertia_tables_get_their_own_key_and_struct():
    gi, _ = fixture("ur5")
    plain = {k: v for k, v in gi.items() if k not in ("mlink", "mjoint")}
    assert _abi.is_general_inertia(gi)
    assert bytes(_abi.desc_from_table(gi)) == bytes(_abi.desc_from_table(plain))
    assert specialize.arm_key(gi, abi="x") != specialize.arm_key(plain, abi="x")
    src = _abi.render_tab_struct(gi, "Tab_x")
    assert "kGI = true" in src and "ML[7][36]" in src and "MJ[6][36]" in src
    assert "kGI" not in _abi.render_tab_struct(plain, "Tab_x")
    # one ulp of one joint inertia is another arm
    g2 = json.loads(json.dumps(gi))
    g2["mjoint"][3][5][5] = np.nextafter(g2["mjoint"][3][5][5], 1.0)
    assert specialize.arm_key(g2, abi="x") != specialize.arm_key(gi, abi="x")


def test_inconsistent_or_asymmetric_inertias_are_refused():
    from abr_control_amd import arms

    gi, _ = fixture("synthetic4")
    bad = json.loads(json.dumps(gi))
    bad["mlink"][2][0][5] += 0.01
    with pytest.raises(ValueError, match="not symmetric"):
        _abi.normalize_table(bad)
    with pytest.raises(ValueError, match="not symmetric"):
        arms.from_table(bad)
    diag = json.loads(json.dumps(_abi.load_table("ur5")))
    diag["mlink"] = [np.diag(r).tolist() for r in diag["mdiag"]]
    diag["mlink"][3][0][0] += 0.5
    with pytest.raises(ValueError, match="differs from mdiag"):
        arms.from_table(diag)
    short = dict(gi, mjoint=gi["mjoint"][:3])
    with pytest.raises(ValueError, match="mjoint"):
        _abi.normalize_table(short)


def test_inertia_struct_layout():
    """ctypes mirror of include/abrk_types.h abrk_arm_inertia: 8 link and 7 joint matrices of 36 doubles"""
    assert C.sizeof(_abi.ArmInertia) == (8 + 7) * 36 * 8
    assert _abi.ArmInertia.mlink.offset == 0 and _abi.ArmInertia.mjoint.offset == 8 * 36 * 8
    gi, _ = fixture("synthetic4")
    x = _abi.inertia_from_table(gi)
    a = np.frombuffer(bytes(x), dtype=np.float64)
    assert np.array_equal(a[: 5 * 36].reshape(5, 6, 6), np.array(gi["mlink"]))
    assert np.array_equal(a[8 * 36: 12 * 36].reshape(4, 6, 6), np.array(gi["mjoint"]))
    assert not a[5 * 36: 8 * 36].any() and not a[12 * 36:].any()


@pytest.mark.parametrize("arm", ARMS)
def test_host_row_programs_match_the_reference(arm):
    """the row programs (abrk_rows.h dyn_body; Dyn CMODE_VEC for the fused laws' C dq) built for the host on the
    general-inertia table, against the reference's SymPy M, g, C at 1e-10 relative"""
    from tests import hostsim_gi

    tab, z = fixture(arm)
    q, dq = z["dyn_q"], z["dyn_dq"]
    want = ("M", "g", "C") if "C" in z.files else ("M", "g")
    r = hostsim_gi.dynamics(tab, q, dq, want=want)
    for k in want:
        err = np.max(np.abs(r[k] - z[k])) / np.max(np.abs(z[k]))
        assert err < 1e-10, f"{arm} {k}: {err:.2e}"
    if "C" in z.files:
        ref = np.einsum("bij,bj->bi", z["C"], dq)
        cv = hostsim_gi.coriolis_vector(tab, q, dq)
        assert np.max(np.abs(cv - ref)) / np.max(np.abs(ref)) < 1e-10


def test_general_inertia_arm_runs_compiled_only():
    """from_table on a general-inertia table takes the compiled plugin (built by build(), in-tree cache), registers its
    inertias with it, and refuses the runtime-table path; the plugin refuses the plain description"""
    from abr_control_amd import arms
    from abr_control_amd._lib import check, lib

    for arm in ARMS:
        tab, _ = fixture(arm)
        rc = arms.from_table(tab)
        assert rc.general_inertia and rc.arm_id >= 5
        assert rc.plugin_path == specialize.find_compiled(tab) and rc.plugin_path.startswith(specialize.IN_TREE)
        got = _abi.ArmInertia()
        check(lib().abrk_arm_get_inertia(rc.arm_id, C.byref(got)))
        assert bytes(got) == bytes(_abi.inertia_from_table(tab))
        np.testing.assert_array_equal(rc._M_JOINTS[1], np.array(tab["mjoint"][1]))
        # the plain description alone does not match the plugin's inertias
        d = _abi.desc_from_table(tab)
        assert lib().abrk_arm_create_compiled(C.byref(d), rc.plugin_path.encode()) == -1
        assert b"inertias" in lib().abrk_last_error()
        with pytest.raises(ValueError, match="compiled kernels only"):
            arms.from_table(tab, compiled=False)
        rc.close()
    # plain arms report the plain form
    ur5 = check(lib().abrk_arm_builtin(b"ur5"))
    got = _abi.ArmInertia()
    check(lib().abrk_arm_get_inertia(ur5, C.byref(got)))
    assert bytes(got) == bytes(_abi.inertia_from_table(_abi.load_table("ur5")))
