"""A mesh of an element family outside the table of instantiated families (npe = 5, dm = 3: femcy_set_mesh takes any npe
of 2 .. 27, so the mesh is accepted and the call reaches the dispatch): every entry point that selects an element
instantiation fails with FEMCY_ENOKERNEL and its own message, and hands out no object."""
import numpy as np
import pytest

import loads_reference as lr
from femcy_amd import backend as be
from femcy_amd.material_zoo import LinearIsotropic

FEMCY_ENOKERNEL = -3
NPE, DM = 5, 3


class Pyramid5:
    """tables of a family no kernel is instantiated for: one Gauss point, arbitrary finite dN / N (seeded)"""
    npe, dm = NPE, DM

    def __init__(self):
        rng = np.random.default_rng(5)
        self.dN = rng.uniform(-1.0, 1.0, (1, NPE, DM))
        self.N = rng.uniform(0.1, 0.3, (1, NPE))

    def tables(self):
        return {"nGP": 1, "npe": NPE, "dm": DM, "dN": self.dN, "N": self.N, "w": np.array([0.5]), "voigt_kind": 1}

    def mass_tables(self):
        return {"nq": 1, "Nq": self.N, "dNq": self.dN, "wq": np.array([0.5])}


def _refused_ctx(make):
    """two elements on 6 nodes, through femcy_build_pattern"""
    nodes = np.random.default_rng(6).uniform(0.0, 1.0, (6, DM))
    el = np.array([[0, 1, 2, 3, 4], [1, 2, 3, 4, 5]], dtype=np.int32)
    ELE = Pyramid5()
    assert ELE.tables()["voigt_kind"] == lr.single("C3D4")[2].tables()["voigt_kind"]
    ctx = make()
    ctx.set_mesh(nodes, el)
    ctx.set_element(ELE)
    ctx.set_material(LinearIsotropic(2.0e5, 0.3))
    ctx.build_pattern()
    return ctx, ELE


def _refusals(ctx, ELE, geometry):
    """(call, exact message) of every dispatched entry point, then: no id was handed out"""
    calls = [(lambda: ctx.bodyload(ELE), "no body-load kernel instantiated for npe=5 dm=3"),
             (lambda: ctx.thermal(ELE, 1.2e-5, np.linspace(10.0, 60.0, ctx.nn)),
              "no thermal-load kernel instantiated for npe=5 dm=3"),
             (lambda: ctx.mass(ELE, 7.85e-3), "no mass kernel instantiated for npe=5 dm=3")]
    if geometry:
        calls.append((lambda: ctx.internal_force(be.VEC_DOF, be.VEC_FORCE),
                      "no geometry kernel instantiated for npe=5 dm=3"))
    for call, text in calls:
        with pytest.raises(be.FemcyError) as err:
            call()
        assert err.value.status == FEMCY_ENOKERNEL
        assert str(err.value).endswith(f"-> {FEMCY_ENOKERNEL}: {text}"), str(err.value)
    for call, text in ((lambda: ctx.bodyload_apply(0, [0.0, 0.0, -9.81]), "unknown body load 0"),
                       (lambda: ctx.thermal_apply(0, 1.0), "unknown thermal load 0"),
                       (lambda: ctx.mass_apply(0, be.VEC_VEL, be.VEC_RHS), "unknown mass object 0")):
        with pytest.raises(be.FemcyError) as err:
            call()
        assert str(err.value).endswith(": " + text), str(err.value)


def _first_ids_of_a_valid_family(make):
    """the next context of an instantiated family starts its objects at id 0"""
    nodes, el, ELE, _ = lr.single("C3D4")
    ctx = make()
    ctx.set_mesh(nodes, el)
    ctx.set_element(ELE)
    ctx.set_material(LinearIsotropic(2.0e5, 0.3))
    ctx.build_pattern()
    assert ctx.bodyload(ELE) == 0
    assert ctx.thermal(ELE, 1.2e-5, np.ones(ctx.nn)) == 0
    assert ctx.mass(ELE, 7.85e-3) == 0
    ctx.bodyload_apply(0, [0.0, 0.0, -9.81])
    ctx.thermal_apply(0, 1.0)
    ctx.mass_apply(0, be.VEC_VEL, be.VEC_RHS)


def test_host_backend_refuses_a_family_outside_the_table():
    made = []

    def make():
        made.append(be.Context(0, backend="cpu"))
        return made[-1]

    try:
        ctx, ELE = _refused_ctx(make)
        _refusals(ctx, ELE, geometry=False)      # the host's geometry pass takes npe at run time
        _first_ids_of_a_valid_family(make)
    finally:
        for c in made:
            c.close()


@pytest.mark.gpu
def test_device_refuses_a_family_outside_the_table(gpu_ctx_factory):
    ctx, ELE = _refused_ctx(gpu_ctx_factory)
    _refusals(ctx, ELE, geometry=True)
    _first_ids_of_a_valid_family(gpu_ctx_factory)
