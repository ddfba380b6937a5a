"""Abaqus/CalculiX `.inp` reader, call-compatible with the reference's `InpInfo`
(/root/reference/reader/inp_info.py:14-368) but Taichi-free and single-pass per section.

Attributes after construction (inp_info.py:18-25): nodes, eSets, ELE, node_sets, ele_sets,
face_sets, dirichlet_bc_info, neumann_bc_info, materials, geometric_nonlinear, time_incs.

Reference behaviours that are kept on purpose:
  * only the first `*Node` block is read; node labels are renumbered 0.. in file order (:353-368);
  * the element type is found by substring test in a fixed list order, so CPS6M -> CPS6 (:66-75), and C3D8R /
    C3D8I read as C3D8 with full 2 x 2 x 2 integration (no hourglass control, no incompatible modes);
  * only `*Nset`/`*Elset` keyword lines that contain "instance" are kept; `generate` expands
    start,stop,step inclusively (:142-163);
  * `*Surface` data lines `elset, S<k>` map through ELE.inp_surface_num[k-1]; a face set is a
    set of sorted global-node tuples (:199-212);
  * `*Boundary` data `set, d1[, d2[, val]]`: only d1 is used, val = 4th column or 0; the block is
    "user" when the keyword line contains "user"; every block in the file counts (:218-244);
  * `*Dsload` with <= 3 columns is a pressure: traction = -value along the outward normal; with
    more columns traction = value and direction = columns 3..5 (:246-271);
  * `nlgeom` comes from the last comma field of the first `*Step` line (:319-330); the `amplitude=` parameter added here
    is skipped by that rule;
  * `*Static` data -> ini_inc, max_time, min_inc, max_inc with ini_inc clipped to max_inc (:333-350);
  * 2-D elements accept only `*Elastic`; C3D* accept `*Elastic` and `*Hyperelastic, neo hooke`
    with D1 = 1/value (:294-316).

Beyond the reference (it reads `*Dsload` only and skips the rest): `*Density` inside a `*Material` block -> density,
`*Dload` GRAV / BX / BY / BZ -> body_force_info, `*Cload` -> cload_info (read_loads).  Any other `*Dload` type is
refused by name instead of being skipped.  `*Expansion` inside a `*Material` block -> expansion (isotropic, constant),
`*Initial Conditions, type=TEMPERATURE` and `*Temperature` -> temperature_info (read_thermal).
`*Dynamic, direct[, beta=, gamma=]` with data `dt, T` -> procedure = "dynamic", dynamic = {"beta", "gamma"} and time_incs
with fixed increments (read_procedure); `*Step, amplitude=RAMP|STEP` -> amplitude; `*Initial Conditions, type=VELOCITY` ->
initial_velocity_info.  `*Dynamic, explicit[, direct user control][, scale factor=][, output_every=]` with data `, T` (`dt, T`
under direct user control) -> procedure = "explicit", dynamic = {"direct_user_control", "scale_factor", "output_every"} and
time_incs whose increments are None until the driver has estimated one; `element by element` in place of `direct user
control` -> dynamic_auto = True: the driver re-estimates the increment in every step.  `*Bulk Viscosity` (data `b1, b2`,
defaults 0.06, 1.2) inside an explicit step -> bulk_viscosity = (b1, b2), None without the keyword; `*Damping, alpha=` in the
`*Material` block -> damping_alpha (read_damping).  `*Fixed Mass Scaling[, factor=][, dt=][, type=]` inside an explicit step ->
mass_scaling = {"factor", "dt", "type"}, None without the keyword (read_mass_scaling).  `*Energy Output` inside an explicit
step, alone or under `*Output, history` -> energy_output = True, False without the keyword (read_energy_output).  `*Rigid Wall[, penalty=kappa]` inside an
explicit step, data `x0, y0[, z0], nx, ny[, nz]` -> rigid_walls = [{"point", "normal", "penalty"}] (read_rigid_walls): an
EXTENSION keyword, Abaqus has none for a planar rigid wall.  A deck with `*Static` has procedure = "static" and reads as
before.
"""
import sys
from typing import Dict, List

import numpy as np

from ..element_zoo import (Element_linear_triangular, Element_linear_quadrilateral,
                           Element_quadratic_triangular, Element_quadratic_quadrilateral,
                           Element_linear_tetrahedral, Element_quadratic_tetrahedral, Element_linear_hexahedral,
                           Element_linear_wedge)
from ..material_zoo import (LinearIsotropic, LinearIsotropicPlaneStrain, LinearIsotropicPlaneStress, NeoHookean)
from .inp_info_base import InpInfoBase

# scan order matters: the first type whose name is a substring of the keyword line wins
_TYPE_SCAN_ORDER = ["C3D8", "C3D20", "C3D4", "C3D10", "B31", "C3D6", "CPS3", "CPE3", "CPE4", "CPS4",
                    "CPE8", "CPS8", "CPS6", "CPE6"]
# (integers per record, slice of node columns kept)
_RECORD = {"C3D8": (9, slice(1, 9)), "C3D20": (21, slice(1, 9)), "C3D4": (5, slice(1, 5)),
           "CPE4": (5, slice(1, 5)), "CPS4": (5, slice(1, 5)), "CPS8": (9, slice(1, 9)),
           "CPE8": (9, slice(1, 9)), "C3D10": (11, slice(1, 11)), "B31": (3, slice(1, 3)),
           "CPS3": (4, slice(1, 4)), "CPE3": (4, slice(1, 4)), "C3D6": (7, slice(1, 7)),
           "CPS6": (7, slice(1, 7)), "CPE6": (7, slice(1, 7))}
ELEMENT_CLASSES = {"CPE3": Element_linear_triangular, "CPS3": Element_linear_triangular,
                   "CPE4": Element_linear_quadrilateral, "CPS4": Element_linear_quadrilateral,
                   "CPS6": Element_quadratic_triangular, "CPE6": Element_quadratic_triangular,
                   "CPS8": Element_quadratic_quadrilateral, "CPE8": Element_quadratic_quadrilateral,
                   "C3D4": Element_linear_tetrahedral, "C3D10": Element_quadratic_tetrahedral,
                   "C3D8": Element_linear_hexahedral, "C3D6": Element_linear_wedge}


class _Deck:
    """the file, read once: its lines and the positions of the lines that contain '*' (keyword and comment lines).
    Data blocks are the runs between two such lines, so the section readers below visit keyword lines only and
    hand whole data blocks to numpy -- at 1e6 elements the per-line Python loops of the reference
    (inp_info.py:28-113) were the wall-clock, not the solve."""

    def __init__(self, path):
        with open(path, "r") as fh:
            self.lines = fh.read().split("\n")
        self.star = [i for i, line in enumerate(self.lines) if "*" in line]
        self.star.append(len(self.lines))            # sentinel: end of file closes the last block

    def keywords(self):
        """(keyword line, its data lines) for every non-comment keyword line, in file order.  Comment lines are
        transparent (the data of a keyword continue after a `**` line, as in the reference's line loops); a
        '*' inside a data line ends the block."""
        lines, star = self.lines, self.star
        k, last = 0, len(star) - 1
        while k < last:
            line = lines[star[k]]
            if line[0] == "*" and not _is_comment(line):
                block = lines[star[k] + 1:star[k + 1]]
                j = k + 1
                while j < last and _is_comment(lines[star[j]]):
                    block = block + lines[star[j] + 1:star[j + 1]]
                    j += 1
                yield line, block
                k = j
            else:
                k += 1


_deck_cache = {}


def _deck(path) -> "_Deck":
    import os
    st = os.stat(path)
    key = (os.path.abspath(path), st.st_mtime_ns, st.st_size)
    if key not in _deck_cache:
        _deck_cache.clear()                            # one deck at a time
        _deck_cache[key] = _Deck(path)
    return _deck_cache[key]


def _lines(path):
    return _deck(path).lines


def _numbers(block, dtype):
    """all comma-separated numbers of a data block (trailing commas and blank lines tolerated)."""
    body = ",".join(t for t in (line.rstrip().rstrip(",") for line in block) if t)
    return np.fromstring(body, dtype=dtype, sep=",") if body else np.zeros(0, dtype=dtype)


def _is_comment(line):
    return line[0:2] == "**"


class InpInfo(InpInfoBase):

    def __init__(self, file, allow_2d_hyperelastic: bool = False) -> None:
        """allow_2d_hyperelastic: accept `*Hyperelastic, neo hooke` on CPE elements (plane-strain neo-Hookean, an
        extension of this build).  Off by default: the reference rejects any non-`*Elastic` material on 2-D elements
        (:296-299) and so does this reader."""
        self.allow_2d_hyperelastic = allow_2d_hyperelastic
        self.nodes, self.eSets = self.read_node_element(file)
        self.node_sets, self.ele_sets = self.read_set(file)
        self.face_sets = self.read_face_set(file)
        self.amplitudes = self.read_amplitudes(file)
        self.dirichlet_bc_info, self.neumann_bc_info = self.get_boundary_condition(file)
        self.materials = self.read_material(file)
        self.density, self.body_force_info, self.cload_info = self.read_loads(file)
        self.expansion, self.temperature_info = self.read_thermal(file)
        self.geometric_nonlinear = self.read_geometric_nonlinear(file)
        self.procedure, self.dynamic, self.amplitude = self.read_procedure(file)
        self.time_incs = self.read_time_inc(file)
        self.bulk_viscosity, self.damping_alpha = self.read_damping(file)
        self.mass_scaling = self.read_mass_scaling(file)
        self.energy_output = self.read_energy_output(file)
        self.rigid_walls = self.read_rigid_walls(file)
        self.initial_velocity_info = self.read_initial_velocity(file)

    # ------------------------------------------------------------------ nodes and elements
    def read_node_element(self, fileName):
        deck = _deck(fileName)
        lines, star = deck.lines, deck.star
        labels, coords = np.zeros(0, dtype=np.int64), np.zeros((0, 3))
        for k in range(len(star) - 1):                       # the first *Node block only (reference :28-45)
            line = lines[star[k]]
            if ("*Node" in line) or ("*NODE" in line) or ("*node" in line):
                block = [t for t in lines[star[k] + 1:star[k + 1]] if t.strip()]
                if block:
                    width = block[0].count(",") + 1
                    rec = _numbers(block, np.float64).reshape(-1, width)
                    labels, coords = rec[:, 0].astype(np.int64), np.ascontiguousarray(rec[:, 1:])
                break

        tokens: Dict[str, List[np.ndarray]] = {}
        for k in range(len(star) - 1):
            line = lines[star[k]]
            if ("*ELEMENT" in line) or ("*Element" in line) or ("*element" in line):
                if ("TYPE=" in line) or ("type=" in line):
                    current = next((t for t in _TYPE_SCAN_ORDER if t in line), None)
                    if current is not None:
                        tokens.setdefault(current, []).append(_numbers(lines[star[k] + 1:star[k + 1]], np.int64))
        if len(tokens) > 1:
            print("\033[31;1m there are multiple element types in the file: {} \033[0m".format(list(tokens)))

        eSets = {}
        for eType, toks in tokens.items():
            if eType not in _RECORD:
                print("\033[31;1m Error, element type {} is not found! \033[0m".format(eType))
                sys.exit(1)
            width, keep = _RECORD[eType]
            eSets[eType] = np.concatenate(toks).reshape((-1, width))[:, keep]

        nodes, eSets = self.sequence_order_of_body((labels, coords), eSets)
        first = list(eSets.keys())[0]
        if first not in ELEMENT_CLASSES:
            raise ValueError("element type {} has no element class in element_zoo".format(first))
        self.ELE = ELEMENT_CLASSES[first]()
        if len(eSets) != 1:
            raise ValueError("\033[31;1m multiple element types have not been supported now \033[0m")
        return nodes, eSets

    def sequence_order_of_body(self, nodes, eSets):
        """node labels -> 0-based positions in file order; connectivity renumbered accordingly."""
        if isinstance(nodes, dict):                           # the reference's calling convention (:353-368)
            labels = np.fromiter(nodes.keys(), dtype=np.int64, count=len(nodes))
            coords = np.array(list(nodes.values()), dtype=np.float64)
        else:
            labels, coords = nodes
            _, first = np.unique(labels, return_index=True)   # a repeated label keeps its first position and
            if first.size != labels.size:                     # its last coordinates, as a dict would
                keep = np.sort(first)
                last = {int(l): i for i, l in enumerate(labels)}
                coords = coords[[last[int(l)] for l in labels[keep]]]
                labels = labels[keep]
        lut = np.full(int(labels.max()) + 1, -1, dtype=np.int64)
        lut[labels] = np.arange(labels.size)
        self._label_lut = lut                                 # *Cload with a bare node label goes through the same map
        for eType in eSets:
            eSets[eType] = lut[eSets[eType]]
        return coords, eSets

    # --------------------------------------------------------------------------------- sets
    def read_set(self, fileName):
        node_sets, ele_sets = {}, {}
        for line, block in _deck(fileName).keywords():
            fields = line.split(",")
            if fields[0] in ("*Nset", "*Elset") and "instance" in line:
                store = node_sets if fields[0] == "*Nset" else ele_sets
                name = fields[1].split("=")[1]
                store[name] = set()                  # a repeated name starts over, as in the reference
                if "generate" in fields[-1]:
                    for data_line in block:
                        if data_line:
                            d = _numbers([data_line], np.int64)
                            store[name].update(np.arange(d[0], d[1] + d[2], d[2]).tolist())
                else:
                    store[name].update(_numbers(block, np.int64).tolist())
        as_array = lambda s: np.array(sorted(s), dtype=np.int64) - 1
        return {k: as_array(v) for k, v in node_sets.items()}, {k: as_array(v) for k, v in ele_sets.items()}

    def read_face_set(self, fileName):
        if not hasattr(self, "eSets"):
            self.nodes, self.eSets = self.read_node_element(fileName)
        raw: Dict[str, List[tuple]] = {}
        for line, block in _deck(fileName).keywords():
            fields = line.split(",")
            if fields[0] == "*Surface":
                name = fields[2].split("=")[1]
                raw[name] = []
                for data_line in block:
                    if data_line:
                        f = data_line.split(",")
                        raw[name].append((f[0], f[1]))

        ele_sets = self.ele_sets if hasattr(self, "ele_sets") else self.read_set(fileName)[1]
        conn = self.eSets[list(self.eSets.keys())[0]]
        face_sets = {}
        for sname, entries in raw.items():
            faces = set()
            for elset, tag in entries:
                k = int(tag.split("S")[1]) - 1
                for local in self.ELE.inp_surface_num[k]:
                    keys = np.sort(conn[ele_sets[elset]][:, list(local)], axis=1)
                    faces.update(map(tuple, keys.tolist()))
            face_sets[sname] = faces
        return face_sets

    # ------------------------------------------------------------------ boundary conditions
    def read_amplitudes(self, fileName):
        """`*Amplitude, name=NAME[, definition=TABULAR|SMOOTH STEP]` -> {NAME: {"definition", "t", "A"}}, in step time.
        The data are `t, A` pairs, up to four per line, over any number of lines; 2 to 16 points with increasing times.
        A duplicate name, any other `definition=`, a point count outside that range, an odd number of values and times
        that do not increase are refused."""
        amplitudes = {}
        for line, block in _deck(fileName).keywords():
            fields = [t.strip() for t in line.split(",")]
            if fields[0].lower() != "*amplitude":
                continue
            params = {t.split("=")[0].strip().lower(): t.split("=", 1)[1].strip() for t in fields[1:] if "=" in t}
            name = params.get("name")
            if not name:
                raise ValueError("*Amplitude needs name=")
            if name in amplitudes:
                raise ValueError("*Amplitude, name={} is defined twice".format(name))
            definition = " ".join(params.get("definition", "TABULAR").upper().split())
            if definition not in ("TABULAR", "SMOOTH STEP"):
                raise ValueError("*Amplitude, definition={} has not been supported (TABULAR and SMOOTH STEP are)".format(
                    params["definition"]))
            vals = _numbers(block, np.float64)
            if vals.size % 2:
                raise ValueError("*Amplitude, name={}: the data are `t, A` pairs, {} values were given".format(name, vals.size))
            t, A = vals[0::2].copy(), vals[1::2].copy()
            if not 2 <= t.size <= 16:
                raise ValueError("*Amplitude, name={}: {} points are refused (2 to 16 are taken)".format(name, t.size))
            if not np.all(np.isfinite(vals)) or not np.all(np.diff(t) > 0.0):
                raise ValueError("*Amplitude, name={}: the times must be finite and increasing".format(name))
            amplitudes[name] = {"definition": definition, "t": t, "A": A}
        return amplitudes

    def get_boundary_condition(self, fileName):
        if not hasattr(self, "node_sets"):
            self.node_sets, self.ele_sets = self.read_set(fileName)
        if not hasattr(self, "face_sets"):
            self.face_sets = self.read_face_set(fileName)
        if not hasattr(self, "amplitudes"):
            self.amplitudes = self.read_amplitudes(fileName)
        dirichlet, neumann = [], []
        for line, block in _deck(fileName).keywords():
            if line[0:9] == "*Boundary":
                # `*Boundary, amplitude=NAME` (prescribed motion, *Dynamic, explicit only: read_procedure): the entries gain
                # the key "amplitude"; without the parameter the key is absent and the dictionaries are what they always were
                fields = [t.strip() for t in line.split(",")[1:]]
                named = [t.split("=", 1)[1].strip() for t in fields if t.split("=")[0].strip().lower() == "amplitude" and "=" in t]
                if named:
                    user = any(t.lower() == "user" for t in fields)
                    if user:
                        raise ValueError("*Boundary, amplitude={} together with `user` has not been supported".format(named[0]))
                    if named[0] not in self.amplitudes:
                        raise ValueError("*Boundary, amplitude={}: the deck has no *Amplitude of that name".format(named[0]))
                else:
                    user = "user" in line
                for data_line in block:
                    if data_line:
                        f = data_line.split(",")
                        dirichlet.append({"node_set": self.node_sets[f[0]], "dof": int(f[1]) - 1,
                                          "val": float(f[3]) if len(f) >= 4 else 0., "user": user})
                        if named:
                            dirichlet[-1]["amplitude"] = named[0]
            elif line[0:7] == "*Dsload":
                for data_line in block:
                    if not data_line:
                        continue
                    f = data_line.split(",")
                    if len(f) <= 3:       # pressure: positive value pushes against the outward normal
                        neumann.append({"face_set": self.face_sets[f[0]], "traction": -float(f[2])})
                    else:                 # TRVEC: magnitude + direction
                        neumann.append({"face_set": self.face_sets[f[0]], "traction": float(f[2]),
                                        "direction": np.array([float(t) for t in f[3:6]])})
        return dirichlet, neumann

    # ---------------------------------------------------------------------------- materials
    def read_material(self, fileName):
        raw = {}
        expect_type = False
        for line, block in _deck(fileName).keywords():        # *Material, then the type keyword and its data line
            if line[0:9] == "*Material":
                expect_type = True
            elif line[0:8].lower() == "*density":             # Abaqus/CAE writes it first; it is not the material type
                continue
            elif line[0:10].lower() == "*expansion":          # neither is the expansion coefficient (read_thermal)
                continue
            elif line[0:8].lower() == "*damping":             # nor the damping (read_damping); CAE writes it before *Density
                continue
            elif expect_type:
                expect_type = False
                data = [t for t in block if t]
                if data:
                    raw[line.split("*")[1]] = [float(t) for t in data[-1].split(",")]
        ele_type = list(self.eSets.keys())[0]
        family = ele_type[0:3]
        materials = {}
        for key, vals in raw.items():
            if family == "CPE" and "neo hooke" in key and getattr(self, "allow_2d_hyperelastic", False):
                from ..material_zoo import NeoHookeanPlaneStrain
                materials[key] = NeoHookeanPlaneStrain(C1=vals[0], D1=1. / vals[1])
            elif family in ("CPS", "CPE"):
                if key != "Elastic":
                    raise ValueError("only support linear elastic material for 2d element now.")
                cls = LinearIsotropicPlaneStress if family == "CPS" else LinearIsotropicPlaneStrain
                materials[key] = cls(modulus=vals[0], poisson_ratio=vals[1])
            elif family == "C3D":
                if key == "Elastic":
                    materials[key] = LinearIsotropic(modulus=vals[0], poisson_ratio=vals[1])
                elif "neo hooke" in key:
                    materials[key] = NeoHookean(C1=vals[0], D1=1. / vals[1])
                else:
                    raise ValueError("material type {} has not been supported now".format(key))
        return materials

    # -------------------------------------------------------------------- density and loads
    def read_loads(self, fileName):
        """-> density (float or None), body_force_info, cload_info.
        `*Density` (inside a `*Material` block, before or after the material type): the first number of its data.
        `*Dload` data `[elset], GRAV, g, nx, ny[, nz]` and `[elset], BX|BY|BZ, value` -> {"ele_set": 0-based element
        index array or None (whole mesh), "force": f64[dm] per unit volume}; GRAV gives density * g * n.
        `*Cload` data `nset-or-node-label, dof, value` -> {"node_set", "dof", "val"} like a `*Boundary` entry; a bare
        label is mapped to its position like the connectivity."""
        dm = int(self.ELE.dm)
        density, in_material = None, False
        dloads, cloads = [], []
        for line, block in _deck(fileName).keywords():
            key = line.split(",")[0].strip().lower()
            if key == "*material":
                in_material = True
            elif key == "*density" and in_material:
                data = [t for t in block if t.strip()]
                if not data:
                    raise ValueError("*Density without a data line")
                density = float(data[0].split(",")[0])
            elif key == "*dload":
                dloads += [[t.strip() for t in d.split(",")] for d in block if d.strip()]
            elif key == "*cload":
                cloads += [[t.strip() for t in d.split(",")] for d in block if d.strip()]
        body_force_info = []
        for f in dloads:
            if len(f) < 3:
                raise ValueError("*Dload data line needs `[elset], type, value`: {}".format(", ".join(f)))
            if f[0] and f[0] not in self.ele_sets:
                raise ValueError("*Dload: unknown element set {}".format(f[0]))
            ele_set = self.ele_sets[f[0]] if f[0] else None
            kind = f[1].upper()
            force = np.zeros(dm)
            if kind == "GRAV":
                if density is None:
                    raise ValueError("*Dload GRAV needs a *Density in the *Material block")
                n = [float(t) for t in f[3:6] if t]
                if len(n) < 2:
                    raise ValueError("*Dload GRAV needs `g, nx, ny[, nz]`: {}".format(", ".join(f)))
                n = (n + [0.0])[:3]
                if dm == 2 and n[2] != 0.0:
                    raise ValueError("*Dload GRAV with a z component on a 2-D mesh")
                force[:] = density * float(f[2]) * np.asarray(n[:dm])
            elif kind in ("BX", "BY", "BZ"):
                comp = "XYZ".index(kind[1])
                if comp >= dm:
                    raise ValueError("*Dload BZ on a 2-D mesh")
                force[comp] = float(f[2])
            else:
                raise ValueError("*Dload type {} has not been supported (GRAV, BX, BY, BZ are)".format(f[1]))
            body_force_info.append({"ele_set": ele_set, "force": force})
        cload_info = []
        for f in cloads:
            if len(f) < 3:
                raise ValueError("*Cload data line needs `nset-or-node, dof, value`: {}".format(", ".join(f)))
            if f[0] in self.node_sets:
                node_set = self.node_sets[f[0]]
            else:
                try:
                    label = int(f[0])
                except ValueError:
                    raise ValueError("*Cload: {} is neither a node set nor a node label".format(f[0])) from None
                lut = self._label_lut
                if not (0 <= label < lut.size) or lut[label] < 0:
                    raise ValueError("*Cload: no node with label {}".format(label))
                node_set = np.array([lut[label]], dtype=np.int64)
            dof = int(f[1]) - 1
            if not 0 <= dof < dm:
                raise ValueError("*Cload: degree of freedom {} on a {}-D mesh".format(f[1], dm))
            cload_info.append({"node_set": node_set, "dof": dof, "val": float(f[2])})
        return density, body_force_info, cload_info

    # ------------------------------------------------------------------------- thermal loads
    def _nodes_of(self, keyword, name):
        """a node set by its name, or a bare node label through the label map of the connectivity (like `*Cload`)"""
        if name in self.node_sets:
            return self.node_sets[name]
        try:
            label = int(name)
        except ValueError:
            raise ValueError("{}: {} is neither a node set nor a node label".format(keyword, name)) from None
        lut = self._label_lut
        if not (0 <= label < lut.size) or lut[label] < 0:
            raise ValueError("{}: no node with label {}".format(keyword, label))
        return np.array([lut[label]], dtype=np.int64)

    def read_thermal(self, fileName):
        """-> expansion (float or None), temperature_info ({"initial": f64[nn], "final": f64[nn]} or None).
        `*Expansion` (inside a `*Material` block, before or after the material type): one data line with one number, the
        isotropic, constant coefficient alpha.  `zero=` is accepted: the reference temperature cancels for a constant
        alpha.  `type=ORTHO` / `type=ANISO`, a second data line and a second column (temperature-dependent alpha) are
        refused by name.
        `*Initial Conditions, type=TEMPERATURE` and `*Temperature`: data lines `nset-or-node-label, T`.  A node that
        `*Temperature` does not name keeps its initial value; a missing initial value is 0.  Any other
        `*Initial Conditions` type is left alone.  `*Temperature` without `*Expansion` is an error."""
        expansion, in_material = None, False
        initial_lines, final_lines, seen = [], [], False
        for line, block in _deck(fileName).keywords():
            fields = [t.strip() for t in line.split(",")]
            key = fields[0].lower()
            params = {t.split("=")[0].strip().lower(): t.split("=")[1].strip() for t in fields[1:] if "=" in t}
            if key == "*material":
                in_material = True
            elif key == "*expansion" and in_material:
                kind = params.get("type", "ISO").upper()
                if kind != "ISO":
                    raise ValueError("*Expansion, type={} has not been supported (isotropic expansion is)".format(kind))
                data = [t for t in block if t.strip()]
                if not data:
                    raise ValueError("*Expansion without a data line")
                cols = [t for t in data[0].split(",") if t.strip()]
                if len(data) > 1 or len(cols) > 1:
                    raise ValueError("*Expansion: a temperature-dependent coefficient (more than one data line or a "
                                     "second column) has not been supported")
                expansion = float(cols[0])
            elif key == "*initial conditions":
                if params.get("type", "").upper() == "TEMPERATURE":
                    seen = True
                    initial_lines += [[t.strip() for t in d.split(",")] for d in block if d.strip()]
            elif key == "*temperature":
                seen = True
                final_lines += [[t.strip() for t in d.split(",")] for d in block if d.strip()]
        if not seen:
            return expansion, None
        if final_lines and expansion is None:
            raise ValueError("*Temperature needs an *Expansion in the *Material block")
        initial = np.zeros(len(self.nodes), dtype=np.float64)
        for f in initial_lines:
            if len(f) < 2 or not f[1]:
                raise ValueError("*Initial Conditions, type=TEMPERATURE data line needs `nset-or-node, T`: {}".format(", ".join(f)))
            initial[self._nodes_of("*Initial Conditions", f[0])] = float(f[1])
        final = initial.copy()
        for f in final_lines:
            if len(f) < 2 or not f[1]:
                raise ValueError("*Temperature data line needs `nset-or-node, T`: {}".format(", ".join(f)))
            final[self._nodes_of("*Temperature", f[0])] = float(f[1])
        return expansion, {"initial": initial, "final": final}

    # ---------------------------------------------------------------------- step definition
    def read_geometric_nonlinear(self, fileName) -> bool:
        """the last comma field of the first `*Step` line, as the reference reads it (`nlgeom=NO, inc=100` is nlgeom: kept on
        purpose, tests/test_host_logic.py::test_reader_quirks).  The `amplitude=` parameter, which this reader adds, is
        transparent to that rule: `nlgeom=NO, amplitude=STEP` and `amplitude=STEP, nlgeom=NO` read alike."""
        for line, _ in _deck(fileName).keywords():
            if line[:5] == "*Step":
                fields = [f for f in line.split(",") if not f.strip().lower().startswith("amplitude=")]
                return fields[-1].split("nlgeom=")[-1].rstrip() != "NO" if len(fields) < len(line.split(",")) \
                    else fields[-1].split("nlgeom=")[-1] != "NO"
        raise ValueError("no *Step keyword in {}".format(fileName))

    def read_procedure(self, fileName):
        """-> procedure ("static" | "dynamic"), dynamic ({"beta", "gamma"} or None), amplitude ("RAMP" | "STEP").
        `*Dynamic` needs `direct` (fixed increments; automatic time incrementation is not built), takes the Newmark
        parameters `beta=` / `gamma=` (default 1/4, 1/2: the trapezoidal rule, no numerical damping) and refuses
        `alpha=` other than 0 (no HHT damping), beta <= 0, gamma < 1/2, a deck without `*Density`, and a non-zero
        `*Boundary` value (prescribed motion).  `*Step, amplitude=` defaults to RAMP under `*Static` (every load grows
        with t / T, as it always did) and to STEP under `*Dynamic` (loads in full from t = 0+).
        `*Dynamic, explicit[, direct user control][, scale factor=][, output_every=]` -> procedure "explicit" and dynamic =
        {"direct_user_control", "scale_factor", "output_every"}: central differences with a lumped mass (`solve_explicit`).
        It refuses `beta=` / `gamma=` / `alpha=`, a deck without `*Density`, a non-zero `*Boundary` value that names no
        `*Amplitude` (a jump is not a motion; with `amplitude=NAME` the entry is prescribed motion, and that parameter is
        refused under `*Static` and `*Dynamic, direct`, where it is not built) and `*Temperature`.`element by element` on `*Dynamic, explicit` asks for the increment to be re-estimated from the
        current configuration in every step; it is refused together with `direct user control` and on any other
        `*Dynamic`.  The flag is kept beside the dictionary, as `self.dynamic_auto` (False for every other deck)."""
        procedure, dynamic, amplitude = "static", None, None
        self.dynamic_auto = False
        for line, block in _deck(fileName).keywords():
            fields = [t.strip() for t in line.split(",")]
            key = fields[0].lower()
            params = {t.split("=")[0].strip().lower(): t.split("=")[1].strip() for t in fields[1:] if "=" in t}
            flags = {t.lower() for t in fields[1:] if "=" not in t}
            if key == "*step" and amplitude is None and "amplitude" in params:
                amplitude = params["amplitude"].upper()
                if amplitude not in ("RAMP", "STEP"):
                    raise ValueError("*Step, amplitude={} has not been supported (RAMP and STEP are)".format(params["amplitude"]))
            elif key == "*dynamic" and "explicit" in flags:
                for name in ("beta", "gamma", "alpha"):
                    if name in params:
                        raise ValueError("*Dynamic, explicit, {}= has not been supported: central differences have no "
                                         "Newmark or HHT parameter".format(name))
                scale_factor, output_every = float(params.get("scale factor", 1.0)), int(params.get("output_every", 64))
                if not scale_factor > 0.0 or output_every < 1:
                    raise ValueError("*Dynamic, explicit: scale factor = {} and output_every = {} are refused (both must "
                                     "be positive)".format(scale_factor, output_every))
                if "element by element" in flags and "direct user control" in flags:
                    raise ValueError("*Dynamic, explicit: `element by element` estimates the increment in every step and "
                                     "`direct user control` fixes it; give one of them")
                self.dynamic_auto = "element by element" in flags
                procedure = "explicit"
                dynamic = {"direct_user_control": "direct user control" in flags, "scale_factor": scale_factor,
                           "output_every": output_every}
                break
            elif key == "*dynamic":
                if "element by element" in flags:
                    raise ValueError("*Dynamic, element by element has not been supported without `explicit`: the "
                                     "implicit integrator takes fixed increments")
                if "direct" not in flags:
                    raise ValueError("*Dynamic without `direct` has not been supported: automatic time incrementation "
                                     "is not built, give fixed increments with *Dynamic, direct")
                if float(params.get("alpha", 0.0)) != 0.0:
                    raise ValueError("*Dynamic, alpha={} has not been supported: the integrator is the undamped Newmark "
                                     "scheme (alpha = 0)".format(params["alpha"]))
                beta, gamma = float(params.get("beta", 0.25)), float(params.get("gamma", 0.5))
                if not beta > 0.0 or not gamma >= 0.5:
                    raise ValueError("*Dynamic: beta = {} and gamma = {} are refused (beta > 0 and gamma >= 1/2 are "
                                     "needed)".format(beta, gamma))
                procedure, dynamic = "dynamic", {"beta": beta, "gamma": gamma}
                break
            elif key == "*static":
                break
        if procedure in ("dynamic", "explicit"):
            if getattr(self, "density", None) is None:
                raise ValueError("*Dynamic needs a *Density in the *Material block")
            if any(bc["val"] != 0.0 and "amplitude" not in bc for bc in self.dirichlet_bc_info):
                raise ValueError("a non-zero *Boundary value in a *Dynamic step (prescribed motion) has not been supported")
        if procedure != "explicit":
            for bc in self.dirichlet_bc_info:
                if "amplitude" in bc:
                    raise ValueError("*Boundary, amplitude={} has not been supported in a *{} step: prescribed motion is "
                                     "built for *Dynamic, explicit alone".format(
                                         bc["amplitude"], "Static" if procedure == "static" else "Dynamic, direct"))
        if procedure == "explicit" and getattr(self, "temperature_info", None) is not None:
            raise ValueError("*Temperature in a *Dynamic, explicit step has not been supported: thermal loads are small "
                             "strain, an explicit step is not")
        return procedure, dynamic, amplitude or ("RAMP" if procedure == "static" else "STEP")

    def read_damping(self, fileName):
        """-> bulk_viscosity ((b1, b2) or None), damping_alpha.  `*Bulk Viscosity` inside the step, data line `b1, b2`; an
        absent line or an empty field gives Abaqus's defaults 0.06 and 1.2.  Without the keyword there is NO bulk viscosity
        (None): unlike Abaqus/Explicit, where it is on by default, so that existing decks keep their results.
        `*Damping, alpha=` in the `*Material` block: mass-proportional damping, 0.0 without it.  `beta=` other than 0,
        `composite=` and `structural=` are refused (stiffness-proportional damping is not built), negative values too, and
        either keyword in a deck whose procedure is not "explicit": the implicit integrator is undamped."""
        bulk, alpha = None, 0.0
        for line, block in _deck(fileName).keywords():
            fields = [t.strip() for t in line.split(",")]
            key = fields[0].lower()
            params = {t.split("=")[0].strip().lower(): t.split("=")[1].strip() for t in fields[1:] if "=" in t}
            if key == "*bulk viscosity":
                data = [t for t in block if t.strip()]
                cols = [t.strip() for t in data[0].split(",")] if data else []
                b1 = float(cols[0]) if len(cols) > 0 and cols[0] else 0.06
                b2 = float(cols[1]) if len(cols) > 1 and cols[1] else 1.2
                if not (b1 >= 0.0 and b2 >= 0.0 and np.isfinite(b1) and np.isfinite(b2)):
                    raise ValueError("*Bulk Viscosity: b1 = {} and b2 = {} are refused (neither may be negative)".format(b1, b2))
                bulk = (b1, b2)
            elif key == "*damping":
                for name in ("composite", "structural"):
                    if name in params:
                        raise ValueError("*Damping, {}= has not been supported: mass-proportional damping (alpha=) "
                                         "is".format(name))
                if float(params.get("beta", 0.0)) != 0.0:
                    raise ValueError("*Damping, beta={} has not been supported: stiffness-proportional damping is not built, "
                                     "mass-proportional damping (alpha=) is".format(params["beta"]))
                alpha = float(params.get("alpha", 0.0))
                if not (alpha >= 0.0 and np.isfinite(alpha)):
                    raise ValueError("*Damping, alpha={} is refused (it may not be negative)".format(params["alpha"]))
        if self.procedure != "explicit":
            if bulk is not None:
                raise ValueError("*Bulk Viscosity has not been supported outside a *Dynamic, explicit step")
            if alpha != 0.0:
                raise ValueError("*Damping has not been supported outside a *Dynamic, explicit step: the implicit "
                                 "integrator is the undamped Newmark scheme")
        return bulk, alpha

    def read_energy_output(self, fileName):
        """`*Energy Output` inside a `*Dynamic, explicit` step, alone or under `*Output, history` -> True, False without the
        keyword.  The driver then keeps an energy balance of the run and adds it to every record.  Optional data lines name
        variables out of ALLKE, ALLSE, ALLIE, ALLWK, ALLVD and ETOTAL; the whole balance is recorded whichever are named.
        Refused: any other variable, by name, and the keyword in a deck whose procedure is not "explicit"."""
        known = ("ALLKE", "ALLSE", "ALLIE", "ALLWK", "ALLVD", "ETOTAL")
        asked = False
        for line, block in _deck(fileName).keywords():
            if " ".join(line.split(",")[0].lower().split()) != "*energy output":
                continue
            asked = True
            for row in block:
                for name in (t.strip() for t in row.split(",")):
                    if name and name.upper() not in known:
                        raise ValueError("*Energy Output: the variable {} has not been supported ({} are)".format(
                            name, ", ".join(known)))
        if asked and self.procedure != "explicit":
            raise ValueError("*Energy Output has not been supported outside a *Dynamic, explicit step")
        return asked

    def read_rigid_walls(self, fileName):
        """`*Rigid Wall[, penalty=kappa]` inside a `*Dynamic, explicit` step, data lines `x0, y0[, z0], nx, ny[, nz]` ->
        [{"point", "normal", "penalty"}], one entry per data line of every keyword, [] without it.  A frictionless planar
        rigid wall through the point with the normal pointing into the free half space; a node behind it is pushed back by
        the penalty force kappa m (depth) along the normal (`femcy_explicit_set_wall`).  `penalty` is kappa in 1/s^2, None
        without the parameter: the driver then takes 0.1 omega^2 of its first frequency estimate.
        This is an EXTENSION keyword in the spirit of LS-DYNA's planar rigid wall: Abaqus has no single keyword for it (it
        needs an analytical rigid surface, a reference node, a contact pair and a surface interaction).
        Refused: more than 4 walls, the wrong number of fields for the mesh dimension, a zero normal, `penalty <= 0`, and the
        keyword in a deck whose procedure is not "explicit"."""
        dm = int(self.ELE.dm)
        walls = []
        for line, block in _deck(fileName).keywords():
            fields = [t.strip() for t in line.split(",")]
            if " ".join(fields[0].lower().split()) != "*rigid wall":
                continue
            params = {t.split("=")[0].strip().lower(): t.split("=")[1].strip() for t in fields[1:] if "=" in t}
            penalty = float(params["penalty"]) if "penalty" in params else None
            if penalty is not None and not (penalty > 0.0 and np.isfinite(penalty)):
                raise ValueError("*Rigid Wall, penalty={} is refused (it must be positive)".format(params["penalty"]))
            for d in block:
                if not d.strip():
                    continue
                cols = [t for t in (t.strip() for t in d.rstrip().rstrip(",").split(","))]
                if len(cols) != 2 * dm or not all(cols):
                    raise ValueError("*Rigid Wall data line needs {} fields on a {}-D mesh (a point and a normal): {}".format(
                        2 * dm, dm, ", ".join(cols)))
                vals = np.array([float(t) for t in cols])
                if not np.all(np.isfinite(vals)) or not np.linalg.norm(vals[dm:]) > 0.0:
                    raise ValueError("*Rigid Wall: the normal {} is refused (it must have a length)".format(", ".join(cols[dm:])))
                walls.append({"point": vals[:dm].copy(), "normal": vals[dm:].copy(), "penalty": penalty})
        if len(walls) > 4:
            raise ValueError("*Rigid Wall: {} walls have not been supported (at most 4)".format(len(walls)))
        if walls and self.procedure != "explicit":
            raise ValueError("*Rigid Wall has not been supported outside a *Dynamic, explicit step")
        return walls

    def read_mass_scaling(self, fileName):
        """`*Fixed Mass Scaling[, factor=f][, dt=tau][, type=uniform | below min | set equal dt]` inside a `*Dynamic, explicit`
        step -> {"factor": f or None, "dt": tau or None, "type"}, None without the keyword.  The whole model is scaled once,
        at the beginning of the step: every element's mass by f, and / or by what brings its estimated stable increment to tau
        (`below min`, the default: only the elements below tau; `set equal dt`: all of them, which may lighten some;
        `uniform`: one factor, the smallest increment becomes tau).  Refused: `elset=` (whole model only), `*Variable Mass
        Scaling`, neither `factor` nor `dt`, values that are not positive, `type=` without `dt=`, an unknown type, and the
        keyword in a deck whose procedure is not "explicit"."""
        scaling = None
        for line, block in _deck(fileName).keywords():
            fields = [t.strip() for t in line.split(",")]
            key = " ".join(fields[0].lower().split())
            params = {t.split("=")[0].strip().lower(): t.split("=")[1].strip() for t in fields[1:] if "=" in t}
            if key == "*variable mass scaling":
                raise ValueError("*Variable Mass Scaling has not been supported: the mass is scaled once, at the beginning of "
                                 "the step (*Fixed Mass Scaling)")
            if key != "*fixed mass scaling":
                continue
            if "elset" in params:
                raise ValueError("*Fixed Mass Scaling, elset={} has not been supported: the whole model is scaled".format(
                    params["elset"]))
            if "factor" not in params and "dt" not in params:
                raise ValueError("*Fixed Mass Scaling needs factor=, dt= or both")
            factor = float(params["factor"]) if "factor" in params else None
            dt = float(params["dt"]) if "dt" in params else None
            for name, val in (("factor", factor), ("dt", dt)):
                if val is not None and not (val > 0.0 and np.isfinite(val)):
                    raise ValueError("*Fixed Mass Scaling, {}={} is refused (it must be positive)".format(name, params[name]))
            if "type" in params and dt is None:
                raise ValueError("*Fixed Mass Scaling, type={} needs dt=: the type says how a target increment is "
                                 "met".format(params["type"]))
            kind = " ".join(params.get("type", "below min").lower().split())
            if kind not in ("uniform", "below min", "set equal dt"):
                raise ValueError("*Fixed Mass Scaling, type={} has not been supported (uniform, below min and set equal dt "
                                 "are)".format(params["type"]))
            scaling = {"factor": factor, "dt": dt, "type": kind}
        if scaling is not None and self.procedure != "explicit":
            raise ValueError("*Fixed Mass Scaling has not been supported outside a *Dynamic, explicit step")
        return scaling

    def read_initial_velocity(self, fileName):
        """`*Initial Conditions, type=VELOCITY` data lines `nset-or-node-label, dof, value` -> [{"node_set", "dof",
        "val"}], resolved like `*Cload`"""
        dm = int(self.ELE.dm)
        out = []
        for line, block in _deck(fileName).keywords():
            fields = [t.strip() for t in line.split(",")]
            if fields[0].lower() != "*initial conditions":
                continue
            params = {t.split("=")[0].strip().lower(): t.split("=")[1].strip() for t in fields[1:] if "=" in t}
            if params.get("type", "").upper() != "VELOCITY":
                continue
            for d in block:
                if not d.strip():
                    continue
                f = [t.strip() for t in d.split(",")]
                if len(f) < 3 or not f[2]:
                    raise ValueError("*Initial Conditions, type=VELOCITY data line needs `nset-or-node, dof, value`: {}".format(", ".join(f)))
                dof = int(f[1]) - 1
                if not 0 <= dof < dm:
                    raise ValueError("*Initial Conditions, type=VELOCITY: degree of freedom {} on a {}-D mesh".format(f[1], dm))
                out.append({"node_set": self._nodes_of("*Initial Conditions", f[0]), "dof": dof, "val": float(f[2])})
        return out

    def read_time_inc(self, fileName):
        for line, block in _deck(fileName).keywords():
            if line[:8].lower() == "*dynamic" and "explicit" in [t.strip().lower() for t in line.split(",")[1:]]:
                # `dt, T` under `direct user control`, else `, T`: the increment is then estimated by the driver (ini_inc None)
                data = [t for t in block if t.strip()]
                cols = [t.strip() for t in data[0].split(",")] if data else []
                fixed = "direct user control" in [t.strip().lower() for t in line.split(",")[1:]]
                if len(cols) < 2 or not cols[1] or (fixed and not cols[0]):
                    raise ValueError("*Dynamic, explicit needs the data line `, T` (`dt, T` with direct user control)")
                dt, tmax = (float(cols[0]) if fixed else None), float(cols[1])
                if not tmax > 0.0 or (fixed and not dt > 0.0):
                    raise ValueError("*Dynamic, explicit: dt and T must be positive")
                return {"ini_inc": dt, "max_time": tmax, "min_inc": dt, "max_inc": dt}
            if line[:8].lower() == "*dynamic":
                data = [t for t in block if t.strip()]
                if not data or len([t for t in data[0].split(",") if t.strip()]) < 2:
                    raise ValueError("*Dynamic needs the data line `dt, T`")
                dt, tmax = [float(t) for t in data[0].split(",") if t.strip()][:2]
                if not (dt > 0.0 and tmax > 0.0):
                    raise ValueError("*Dynamic: dt and T must be positive")
                return {"ini_inc": dt, "max_time": tmax, "min_inc": dt, "max_inc": dt}
            if line[:7] == "*Static":
                data = [t for t in block if t]
                if data:
                    ini, tmax, dmin, dmax = [float(t) for t in data[0].split(",")][:4]
                    return {"ini_inc": min(ini, dmax), "max_time": tmax, "min_inc": dmin, "max_inc": dmax}
                break
        raise ValueError("no *Static data line in {}".format(fileName))
