"""The host driver (femcy_amd/stiffnessMtrx.py) pinned by what it asks of the library: every deck below is solved with a
wrapper round `Context._call`, and the list of calls -- names and scalar arguments -- is compared with the one recorded in
tests/golden/driver_calls.json.  The host backend (tests/test_driver_calls_cpu.py) and the device
(tests/test_gpu_driver_calls.py) run the same code against the same file.

The trace.  One `[name, arg, ...]` per call, from the first call of `solve` to the last of `compute_strain_stress`: a float
is written as `float.hex()`, an int as it is, anything else (a pointer, a `byref`, None) as "*".  An exception that escapes
ends the trace with its type name.  Scalars reach `_call` as Python int and float and everything else as a pointer, so the
trace and the arrays behind the pointers are all the driver hands over; the arrays are what the other tests check.

The golden file was recorded on the host backend from the driver as it stood before its four step loops were folded onto one
load schedule and one initial state, and it is not recorded again from a driver that was changed since: a trace that differs
is a change of behaviour.  `python tests/driver_calls_cases.py --write` records it (two runs give the same bytes)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                                              # run as a script: the package lies one level up
    sys.path.insert(0, ROOT)

from femcy_amd import backend as be

import dynamic_cases as dc
import explicit_auto_cases as eac
import explicit_cases as ec
import explicit_damped_cases as edc
import loads_cases as lc
import thermal_cases as tc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "driver_calls.json")
TWO_INCREMENTS = "0.5, 1., 1e-05, 0.5"
BATCH = 48                  # output_every of the explicit decks: 200 fixed steps are four batches and a clipped one; the
                            # `element by element` decks take 27, 31 and 73 steps on the host, the middle of a batch


# ------------------------------------------------------------------------------------------- the decks
def _fixed(case):
    spec = ec.CASES[case]
    return "*Dynamic, explicit, direct user control, output_every=%d\n%r, %r\n" % (BATCH, spec["dt"], spec["dt"] * spec["steps"])


def _bar_T():
    return ec.CASES["bar"]["dt"] * ec.CASES["bar"]["steps"]


def write_no_load(path):
    """the hanging bar's mesh without its weight: no load of any kind, the top pulled by a non-zero *Boundary"""
    nodes, el = lc.bar_mesh("C3D8")
    nsets = {"foot": np.nonzero(nodes[:, 2] < 1e-12)[0], "top": np.nonzero(nodes[:, 2] > lc.LEN - 1e-12)[0]}
    lc.write_deck(path, nodes, el, "C3D8", nsets, "*Elastic\n%.17g, 0.3\n" % lc.E_BAR,
                  "*Boundary\nfoot, 1, 1\nfoot, 2, 2\nfoot, 3, 3\ntop, 3, 3, 0.01\n", static=TWO_INCREMENTS)


def write_newton(path):
    """the plate of lc.write_neo_hookean_plate on a coarser mesh, linear elastic with nlgeom, in one increment: a modified-Newton
    run of three solves that takes both line searches (the neo-Hookean plate takes ten and more iterations at any load)"""
    from femcy_amd import meshgen
    nodes, el = meshgen.plate_wedge(3, 1, 1, perturb=0.15, seed=4, box=(3.0, 1.0, 0.25))
    nsets = {"clamp": np.nonzero(nodes[:, 0] < 1e-12)[0]}
    lc.write_deck(path, nodes, el, "C3D6", nsets, "*Density\n2.,\n*Elastic\n400., 0.3\n",
                  "*Boundary\nclamp, 1, 1\nclamp, 2, 2\nclamp, 3, 3\n*Dload\n, GRAV, 0.005, 0., 0., -1.\n", nlgeom=True)


def _damped(tmpdir, dynamic):
    return edc.deck_with(tmpdir, "*Bulk Viscosity\n0.1, 1.5\n", "*Damping, alpha=200.\n", dynamic=dynamic)


def _thermal(path, **kw):
    tc.write_thermal_deck(path, "C3D8", "bar", static=TWO_INCREMENTS, extra_step="*Cload\nB, 2, 2.\n", **kw)


def _at(path, write, *args, **kw):
    write(path, *args, **kw)


# name -> writer(path, tmpdir) -> None, or the path it chose itself
DECKS = {
    "static-gravity": lambda p, d: _at(p, lc.write_hanging_bar, "C3D8"),
    "static-thermal-cload": lambda p, d: _thermal(p),
    "static-cold-cload": lambda p, d: _thermal(p, thermal=False),
    "static-no-load": lambda p, d: write_no_load(p),
    "static-newton": lambda p, d: write_newton(p),
    "dynamic-energy": lambda p, d: _at(p, dc.write_energy_deck),
    "dynamic-cload": lambda p, d: _at(p, dc.write_traj_deck, "cload"),
    "dynamic-dsload": lambda p, d: _at(p, dc.write_traj_deck, "dsload"),
    "explicit-bar": lambda p, d: _at(p, ec.write_case_deck, "bar", dynamic=_fixed("bar")),
    "explicit-block": lambda p, d: _at(p, ec.write_case_deck, "block", dynamic=_fixed("block")),
    "explicit-gravity": lambda p, d: _at(p, ec.write_case_deck, "gravity", dynamic=_fixed("gravity")),
    "explicit-estimated": lambda p, d: _at(p, ec.write_case_deck, "bar", dynamic="*Dynamic, explicit, scale factor=0.8\n, %r\n" % _bar_T()),
    "auto-bar-STEP": lambda p, d: _at(p, eac.write_traj_deck, "bar-STEP", every=BATCH),
    "auto-block-RAMP": lambda p, d: _at(p, eac.write_traj_deck, "block-RAMP", every=BATCH),
    "damped-fixed": lambda p, d: _damped(d, _fixed("bar")),
    "damped-auto": lambda p, d: _damped(d, eac.auto_dynamic(_bar_T(), BATCH)),
}


# The refusals of the two dynamic procedures.  The reader refuses these decks before the driver sees them, so each case reads
# a deck the reader accepts and then changes what the driver's own gate looks at: name -> (deck, change(inp, system))
def _no_density(inp, system):
    inp.density = None


def _moving_boundary(inp, system):
    inp.dirichlet_bc_info[0]["val"] = 0.01


def _temperature(inp, system):
    inp.temperature_info = {"initial": np.zeros(len(inp.nodes)), "final": np.ones(len(inp.nodes))}


def _several_ranks(inp, system):
    system.part = object()                                            # what a partitioned run carries


REFUSED = {
    "refused-dynamic-ranks": ("dynamic-energy", _several_ranks, "a *Dynamic step on more than one rank has not been supported: "
                              "the mass matrix is single-rank"),
    "refused-dynamic-density": ("dynamic-energy", _no_density, "*Dynamic needs a *Density in the *Material block"),
    "refused-dynamic-boundary": ("dynamic-cload", _moving_boundary, "a non-zero *Boundary value in a *Dynamic step (prescribed "
                                 "motion) has not been supported"),
    "refused-explicit-ranks": ("explicit-bar", _several_ranks, "a *Dynamic, explicit step on more than one rank has not been "
                               "supported: the lumped mass is single-rank"),
    "refused-explicit-density": ("explicit-bar", _no_density, "*Dynamic needs a *Density in the *Material block"),
    "refused-explicit-boundary": ("explicit-block", _moving_boundary, "a non-zero *Boundary value in a *Dynamic step (prescribed "
                                  "motion) has not been supported"),
    "refused-explicit-temperature": ("explicit-gravity", _temperature, "*Temperature in a *Dynamic, explicit step has not been "
                                     "supported: thermal loads are small strain, an explicit step is not"),
}
CASES = list(DECKS) + list(REFUSED)

# The decks whose trace is the recorded one on the device too, because every count in it (increments, steps, batches) comes
# from the deck and not from the arithmetic of the backend.  Left out: the Newton deck (its iterations and line searches follow
# the residuals) and the increment estimated from the matrix (its step count follows the estimate).  The three `element by
# element` decks are in: their count of batches follows the device's clock, but 27, 31 and 73 steps sit in the middle of a
# batch of 48, and the device gave the recorded traces with the driver the file was recorded from.
DEVICE_CASES = [name for name in DECKS if name not in ("static-newton", "explicit-estimated")] + list(REFUSED)

# the keys of `increments[*]` per procedure
RECORD = ["kinc", "time1", "dt", "converged", "newton_loop"]
ENERGIES = ["kinetic", "strain_energy"]
INCREMENT_KEYS = {"static": RECORD, "dynamic": RECORD + ENERGIES, "explicit": RECORD + ENERGIES,
                  "auto": ["kinc", "time1", "dt", "dt_min", "converged", "newton_loop"] + ENERGIES}


# ------------------------------------------------------------------------------------------- the trace
def _entry(name, args):
    out = [name]
    for a in args:
        if isinstance(a, float):
            out.append(float(a).hex())
        elif isinstance(a, int):
            out.append(int(a))
        else:
            out.append("*")
    return out


def record(name, tmpdir, backend):
    """-> (trace, system, inp, the exception that escaped or None)"""
    from femcy_amd.body import Body
    from femcy_amd.reader import InpInfo
    from femcy_amd.stiffnessMtrx import System_of_equations
    deck, change = (REFUSED[name][0], REFUSED[name][1]) if name in REFUSED else (name, None)
    path = os.path.join(str(tmpdir), "%s.inp" % deck)
    path = DECKS[deck](path, str(tmpdir)) or path
    inp = InpInfo(path)
    body = Body(nodes=inp.nodes, elements=list(inp.eSets.values())[0], ELE=inp.ELE)
    system = System_of_equations(body, list(inp.materials.values())[0], inp.geometric_nonlinear, verbose=False,
                                 ctx=be.Context(0, backend=backend))
    if change is not None:
        change(inp, system)
    trace, inner, raised = [], system.ctx._call, None

    def logged(call, *args):
        trace.append(_entry(call, args))
        return inner(call, *args)

    system.ctx._call = logged
    try:
        system.solve(inp)
        system.compute_strain_stress()
    except Exception as e:                                            # noqa: BLE001 -- the trace says which
        raised = e
        trace.append(type(e).__name__)
    finally:
        system.ctx._call = inner
        system.ctx.close()
    return trace, system, inp, raised


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def first_difference(got, want):
    for k, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return "call %d: %s, recorded %s" % (k, g, w)
    return "%d calls, recorded %d" % (len(got), len(want))


def check(name, tmpdir, backend):
    """the deck's trace is the recorded one; a refusal raises its message before any call, a run leaves the records of its
    procedure behind"""
    trace, system, inp, raised = record(name, tmpdir, backend)
    want = golden()[name]
    print(f"{name} [{backend}]: {len(trace)} calls, recorded {len(want)}")
    assert trace == want, first_difference(trace, want)
    if name in REFUSED:
        assert trace == ["ValueError"] and str(raised) == REFUSED[name][2]
        return len(trace)
    assert raised is None
    kind = "auto" if getattr(inp, "dynamic_auto", False) else inp.procedure
    assert system.increments and all(list(i) == INCREMENT_KEYS[kind] for i in system.increments)
    if inp.procedure != "static":
        assert list(system.initial_energy) == ENERGIES
    return len(trace)


def write_golden():
    import tempfile
    out = {}
    for name in CASES:
        out[name] = record(name, tempfile.mkdtemp(), "cpu")[0]
        print("%-30s %5d calls" % (name, len(out[name])))
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join('"%s": %s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in out.items()) + "\n}\n")
    print("%s: %d bytes" % (GOLDEN, os.path.getsize(GOLDEN)))


if __name__ == "__main__":
    if "--write" in sys.argv:
        write_golden()
