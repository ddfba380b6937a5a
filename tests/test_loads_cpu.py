"""*Density / *Dload / *Cload without a GPU: the reader, the quadrature rules behind the closed forms, and the host
backend (libfemcy_cpu.so, the same per-element function as the device kernel) through tests/loads_cases.py."""
import glob
import os

import numpy as np
import pytest

import loads_cases as lc
import loads_reference as lr
from femcy_amd.reader import InpInfo
from femcy_amd.reader.inp_info_base import InpInfoBase

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECKS = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "decks", "*.inp")))


# ------------------------------------------------------------------------------------------ reader
def _deck(tmp_path, etype="C3D8", material="*Elastic\n2e5, 0.3\n", step="", name="d.inp"):
    nodes, el = lc.bar_mesh(etype)
    path = str(tmp_path / name)
    nsets = {"foot": np.nonzero(nodes[:, -1] < 1e-12)[0], "tip": np.nonzero(nodes[:, -1] > lc.LEN - 1e-12)[0]}
    lc.write_deck(path, nodes, el, etype, nsets, material, "*Boundary\nfoot, 1, 1\n" + step,
                  elsets={"upper": np.arange(len(el) // 2, len(el))})
    return path, nodes, el


def test_density_is_not_the_material_type(tmp_path):
    plain = InpInfo(_deck(tmp_path, name="a.inp")[0])
    first = InpInfo(_deck(tmp_path, material="*Density\n7.8e-3,\n*Elastic\n2e5, 0.3\n", name="b.inp")[0])
    last = InpInfo(_deck(tmp_path, material="*Elastic\n2e5, 0.3\n*Density\n7.8e-3\n", name="c.inp")[0])
    assert plain.density is None and plain.body_force_info == [] and plain.cload_info == []
    for inp in (first, last):
        assert inp.density == 7.8e-3 and isinstance(inp.density, float)
        assert list(inp.materials) == list(plain.materials) == ["Elastic"]
        assert type(inp.materials["Elastic"]) is type(plain.materials["Elastic"])
        assert np.array_equal(inp.materials["Elastic"].C, plain.materials["Elastic"].C)
    flat = InpInfo(_deck(tmp_path, "CPS4", material="*Density\n2.5,\n*Elastic\n2e5, 0.3\n", name="e.inp")[0])
    assert flat.density == 2.5 and list(flat.materials) == ["Elastic"]          # 2-D: no longer refused either
    neo = InpInfo(_deck(tmp_path, material="*Density\n2.,\n*Hyperelastic, neo hooke\n80., 2.5e-3\n", name="f.inp")[0])
    assert neo.density == 2.0 and len(neo.materials) == 1 and "neo hooke" in list(neo.materials)[0]
    for attr in ("density", "body_force_info", "cload_info"):
        assert attr in InpInfoBase.ATTRIBUTES


def test_dload_and_cload_are_read(tmp_path):
    step = ("*Dload\n, GRAV, 9.81, 0., 0., -1.\nupper, GRAV, 2., 1., 0., 0.\n, BX, 3.\nupper, BY, -4.\n, BZ, 5.\n"
            "*Cload\ntip, 3, -12.5\n7, 1, 0.25\n")
    path, nodes, el = _deck(tmp_path, material="*Density\n0.5,\n*Elastic\n2e5, 0.3\n", step=step)
    inp = InpInfo(path)
    upper = np.arange(len(el) // 2, len(el))
    want = [(None, [0, 0, -0.5 * 9.81]), (upper, [1.0, 0, 0]), (None, [3.0, 0, 0]), (upper, [0, -4.0, 0]), (None, [0, 0, 5.0])]
    assert len(inp.body_force_info) == len(want)
    for got, (ele_set, force) in zip(inp.body_force_info, want):
        assert (got["ele_set"] is None) if ele_set is None else np.array_equal(got["ele_set"], ele_set)
        assert got["force"].dtype == np.float64 and np.array_equal(got["force"], np.asarray(force, dtype=np.float64))
    tip = np.nonzero(nodes[:, 2] > lc.LEN - 1e-12)[0]
    assert [sorted(c) for c in inp.cload_info] == [["dof", "node_set", "val"]] * 2
    assert np.array_equal(inp.cload_info[0]["node_set"], tip) and inp.cload_info[0]["dof"] == 2
    assert inp.cload_info[0]["val"] == -12.5
    assert np.array_equal(inp.cload_info[1]["node_set"], [6]) and inp.cload_info[1]["dof"] == 0      # label 7 -> position 6
    assert inp.cload_info[1]["val"] == 0.25
    assert inp.neumann_bc_info == [] and len(inp.dirichlet_bc_info) == 1
    flat = InpInfo(_deck(tmp_path, "CPS4", material="*Density\n2.,\n*Elastic\n2e5, 0.3\n",
                         step="*Dload\n, GRAV, 10., 0., -1.\n, BY, 1.5\n*Cload\ntip, 2, 1.\n", name="flat.inp")[0])
    assert [bf["force"].tolist() for bf in flat.body_force_info] == [[0.0, -20.0], [0.0, 1.5]]


def test_a_bare_label_goes_through_the_label_map(tmp_path):
    """node labels that do not start at 1: the *Cload label maps to the node's position, like the connectivity"""
    path, nodes, el = _deck(tmp_path, step="*Cload\n107, 2, 1.\n")
    text = open(path).read().split("*Element")
    head = text[0].split("*Node\n")
    rows = [r.split(",", 1) for r in head[1].strip().split("\n")]
    head[1] = "".join("%d,%s\n" % (int(a) + 100, b) for a, b in rows)
    body = text[1].split("*End Instance")
    erows = body[0].strip().split("\n")
    conn = "\n".join([erows[0]] + [", ".join([r.split(",")[0]] + [str(int(v) + 100) for v in r.split(",")[1:]])
                                   for r in erows[1:]]) + "\n"
    open(path, "w").write("*Node\n".join(head) + "*Element" + conn + "*End Instance" + body[1])
    inp = InpInfo(path)
    assert np.array_equal(list(inp.eSets.values())[0], el)
    assert np.array_equal(inp.cload_info[0]["node_set"], [6])
    with pytest.raises(ValueError, match="no node with label 7"):
        InpInfo(_deck(tmp_path, step="*Cload\n7777, 2, 1.\n", name="g.inp")[0])


@pytest.mark.parametrize("etype,material,step,word", [
    ("C3D8", "*Elastic\n2e5, 0.3\n", "*Dload\n, GRAV, 9.81, 0., 0., -1.\n", "Density"),
    ("CPS4", "*Elastic\n2e5, 0.3\n", "*Dload\n, BZ, 1.\n", "BZ"),
    ("C3D8", "*Elastic\n2e5, 0.3\n", "*Dload\n, CENTRIF, 1., 0., 0., 0., 0., 0., 1.\n", "CENTRIF"),
    ("C3D8", "*Elastic\n2e5, 0.3\n", "*Dload\nupper, P2, 1.\n", "P2"),
    ("C3D8", "*Elastic\n2e5, 0.3\n", "*Dload\n, ROTA, 1.\n", "ROTA"),
    ("C3D8", "*Elastic\n2e5, 0.3\n", "*Dload\nnowhere, BX, 1.\n", "nowhere"),
    ("C3D8", "*Elastic\n2e5, 0.3\n", "*Cload\nnowhere, 1, 1.\n", "nowhere"),
    ("CPS4", "*Elastic\n2e5, 0.3\n", "*Cload\ntip, 3, 1.\n", "degree of freedom"),
])
def test_reader_refusals(tmp_path, etype, material, step, word):
    with pytest.raises(ValueError, match=word):
        InpInfo(_deck(tmp_path, etype, material, step)[0])


def _parent_materials(inp, path):
    """what the reader made of *Material before *Density existed: the keyword after *Material is the type"""
    keys, expect = [], False
    for line in open(path).read().split("\n"):
        if line[:1] == "*" and line[:2] != "**":
            if line[0:9] == "*Material":
                expect = True
            elif expect:
                expect = False
                keys.append(line.split("*")[1])
    return keys


@pytest.mark.parametrize("path", DECKS, ids=[os.path.basename(p) for p in DECKS])
def test_shipped_decks_read_as_before(path):
    """no shipped deck has the new keywords: the new attributes are empty, and what the new code touches (materials,
    the label map) equals what the unchanged attributes say"""
    text = open(path).read().lower()
    assert "*dload" not in text and "*cload" not in text and "*density" not in text
    inp = InpInfo(path)
    assert inp.density is None and inp.body_force_info == [] and inp.cload_info == []
    # the material keys are the keywords that follow *Material, each once, as the parent's reader took them
    keys = _parent_materials(inp, path)
    assert list(inp.materials) == list(dict.fromkeys(keys))
    el = list(inp.eSets.values())[0]
    assert el.min() == 0 and el.max() == len(inp.nodes) - 1 and inp.ELE.npe == el.shape[1]
    for name in InpInfoBase.ATTRIBUTES:
        assert hasattr(inp, name)
    for bc in inp.dirichlet_bc_info:
        assert sorted(bc) == ["dof", "node_set", "user", "val"]
    for nb in inp.neumann_bc_info:
        assert set(nb) in ({"face_set", "traction"}, {"face_set", "traction", "direction"})


# ------------------------------------------------------------------------- rules behind the closed forms
@pytest.mark.parametrize("etype", lr.ETYPES)
def test_rules_integrate_the_shape_functions_exactly(etype):
    """sum_g N_a(xi_g) w_g equals the exact integral of N_a over the reference element (sympy, rational arithmetic on
    the plug-in's own shapeFunc): on a straight-sided simplex, rectangle, brick or right prism det J is constant, so the
    closed forms of loads_cases.closed_form hold for the rule, not only for the exact integral"""
    import sympy as sp
    ELE = lr.single(etype)[2]
    x, y, z = sp.symbols("x y z")
    nat = [x, y, z][:ELE.dm]
    N = [sp.nsimplify(sp.expand(v), rational=True) for v in ELE.shapeFunc_pyscope(np.array(nat, dtype=object))]
    one = sp.Integer(1)
    if etype in ("CPS3", "CPS6"):
        exact = [sp.integrate(sp.integrate(n, (y, 0, one - x)), (x, 0, 1)) for n in N]
    elif etype in ("CPS4", "CPS8"):
        exact = [sp.integrate(sp.integrate(n, (y, -1, 1)), (x, -1, 1)) for n in N]
    elif etype in ("C3D4", "C3D10"):
        exact = [sp.integrate(sp.integrate(sp.integrate(n, (z, 0, one - x - y)), (y, 0, one - x)), (x, 0, 1)) for n in N]
    elif etype == "C3D8":
        exact = [sp.integrate(sp.integrate(sp.integrate(n, (z, -1, 1)), (y, -1, 1)), (x, -1, 1)) for n in N]
    else:
        # the wedge's natural domain: taken from its own Gauss points (triangle coordinates, then the axis)
        gp = np.asarray(ELE.gaussPoints, dtype=np.float64)
        lo, hi = (-1, 1) if gp[:, 2].min() < 0 else (0, 1)
        exact = [sp.integrate(sp.integrate(sp.integrate(n, (z, lo, hi)), (y, 0, one - x)), (x, 0, 1)) for n in N]
    Ng, _, w = lr.element_tables(ELE)
    rule = (Ng * w[:, None]).sum(axis=0)
    assert abs(float(sum(exact)) - w.sum()) < 1e-15                    # the domain above is the rule's domain
    assert np.abs(rule - np.array([float(v) for v in exact])).max() < 1e-15


# ------------------------------------------------------------------------------------ host backend
@pytest.mark.parametrize("etype", lr.ETYPES)
def test_closed_forms_on_the_host(etype):
    lc.closed_form(etype, "cpu")


@pytest.mark.parametrize("etype", lr.ETYPES)
def test_host_weights_match_the_restatement(etype):
    lc.against_restatement(etype, "cpu")


def test_host_fan_selection_and_bits():
    lc.fan_centre("cpu")
    lc.selections("cpu")


def test_host_dofset_add_and_refusals():
    lc.dofset_add("cpu")
    lc.refusals("cpu")


def test_tables_gain_the_shape_functions():
    for etype in lr.ETYPES:
        ELE = lr.single(etype)[2]
        t = ELE.tables()
        assert t["N"].shape == (t["nGP"], ELE.npe) and np.allclose(t["N"].sum(axis=1), 1.0, atol=1e-15)
        assert np.array_equal(t["N"], lr.element_tables(ELE)[0])


@pytest.mark.parametrize("etype", ["C3D8", "CPS4"])
def test_hanging_bar_on_the_host(tmp_path, etype):
    """the column under its own weight, u_z = -rho g (L z - z^2 / 2) / E: bricks and quadrilaterals are nodally exact
    (nu = 0, consistent loads; a column of tetrahedra or wedges is not: its cross-sections do not stay plane, 2.5 % off
    with C3D4); the bound is the direct solve's own (smoke(): 1e-9)"""
    _, err = lc.hanging_bar(str(tmp_path / "bar.inp"), etype, "cpu")
    print(f"{etype}: relative error {err:.3e}")
    assert err <= 1e-9


def test_density_after_elastic_gives_the_same_bar(tmp_path):
    a, b = str(tmp_path / "a.inp"), str(tmp_path / "b.inp")
    lc.write_hanging_bar(a, "C3D8", density_first=True)
    lc.write_hanging_bar(b, "C3D8", density_first=False)
    assert np.array_equal(lc.solve_deck(a, "cpu")[2], lc.solve_deck(b, "cpu")[2])


def test_cload_equals_dsload_on_the_host(tmp_path):
    lc.cload_equals_dsload(str(tmp_path), "cpu")


def test_loads_scale_with_the_increment_and_old_decks_make_the_old_calls(tmp_path):
    """two increments of a linear deck: the second applies the whole load; a deck without the new keywords never
    reaches the new entry points"""
    path = str(tmp_path / "bar.inp")
    nodes = lc.write_hanging_bar(path, "C3D8")
    text = open(path).read().replace("1., 1., 1e-05, 1.", "0.5, 1., 1e-05, 0.5")
    open(path, "w").write(text)
    _, system, u = lc.solve_deck(path, "cpu")
    assert [i["time1"] for i in system.increments] == [0.5, 1.0]
    ue = lc.hanging_bar_exact(nodes)
    # the matrix of the second increment is assembled on the configuration the first one left (the reference does so in
    # linear runs too), which moves the answer by the order of the strain, rho g L / E = 1.5e-6
    assert np.abs(u - ue).max() <= 1e-5 * np.abs(ue).max()
    assert len(system._bodyloads) == 1                                # cached per element set
    from femcy_amd import backend as be
    seen = []
    orig = be.Context._call

    def spy(self, name, *args):
        seen.append(name)
        return orig(self, name, *args)

    be.Context._call = spy
    try:
        lc.cload_equals_dsload(str(tmp_path), "cpu")
    finally:
        be.Context._call = orig
    assert "femcy_dofset_add" in seen and "femcy_loadset_neumann" in seen
    first_cload = seen.index("femcy_dofset_add")
    assert not any(n.startswith("femcy_bodyload") or n == "femcy_dofset_add" for n in seen[:first_cload])


def test_local_deck_hands_over_element_and_node_sets(tmp_path):
    from femcy_amd import partition
    from femcy_amd.body import Body
    step = "*Dload\nupper, BX, 3.\n, GRAV, 1., 0., 0., -1.\n*Cload\ntip, 3, 2.\n"
    path, nodes, el = _deck(tmp_path, "C3D4", material="*Density\n1.,\n*Elastic\n2e5, 0.3\n", step=step)
    inp = InpInfo(path)
    parts = partition.build_all_parts(inp.nodes, el, 2, axis=2)
    held = []
    for p in parts:
        deck = partition.LocalDeck(inp, p, Body(p.nodes, p.elements, inp.ELE))
        upper, whole = deck.body_force_info
        assert whole["ele_set"] is None and np.array_equal(whole["force"], [0, 0, -1.0])
        assert np.array_equal(np.sort(p.elem_ids[upper["ele_set"]]), np.intersect1d(p.elem_ids, inp.ele_sets["upper"]))
        held.append(upper["ele_set"].size)
        assert np.array_equal(p.l2g[deck.cload_info[0]["node_set"]], np.intersect1d(p.l2g, inp.node_sets["tip"]))
        assert deck.density == 1.0
    assert sum(held) == inp.ele_sets["upper"].size and 0 in held      # the lower rank holds nothing of the set: empty, not None
