"""reader interface: what `System_of_equations.solve` and `main.py` expect from any mesh / boundary-condition /
material reader (the role of /root/reference/reader/inp_info_base.py).  A concrete reader must provide every method
named in `REQUIRED`; the check happens when the subclass is defined, not when it is instantiated."""

REQUIRED = ("read_node_element",        # -> nodes f64[nn, dm], {abaqus_type: connectivity}
            "read_set",                 # -> node sets, element sets (0-based index arrays)
            "read_face_set",            # -> {surface name: set of sorted global-node tuples}
            "get_boundary_condition",   # -> Dirichlet list, Neumann list
            "read_material",            # -> {keyword: material_zoo object}
            "read_geometric_nonlinear", # -> bool (nlgeom)
            "read_time_inc")            # -> {"ini_inc", "max_time", "min_inc", "max_inc"}


class InpInfoBase:
    #: attributes a reader instance exposes after construction
    ATTRIBUTES = ("nodes", "eSets", "ELE", "node_sets", "ele_sets", "face_sets", "dirichlet_bc_info",
                  "neumann_bc_info", "materials", "geometric_nonlinear", "time_incs",
                  # loads beyond the reference's *Dsload: *Density (float or None), *Dload GRAV / BX / BY / BZ as
                  # [{"ele_set": index array or None, "force": f64[dm]}], *Cload as [{"node_set", "dof", "val"}]
                  "density", "body_force_info", "cload_info",
                  # thermal loads: *Expansion (float or None), *Initial Conditions, type=TEMPERATURE + *Temperature as
                  # {"initial": f64[nn], "final": f64[nn]} or None
                  "expansion", "temperature_info",
                  # the step's procedure: "static" | "dynamic" (*Dynamic, direct) | "explicit" (*Dynamic, explicit), its
                  # parameters ({"beta", "gamma"}; {"direct_user_control", "scale_factor", "output_every"}) or None, the load amplitude "RAMP" | "STEP", *Initial Conditions, type=VELOCITY as [{"node_set", "dof", "val"}]
                  # dynamic_auto: `element by element` on *Dynamic, explicit (bool; kept beside the dictionary)
                  "procedure", "dynamic", "amplitude", "initial_velocity_info", "dynamic_auto",
                  # damping of an explicit step: *Bulk Viscosity as (b1, b2) or None, *Damping, alpha= (0.0 without it)
                  "bulk_viscosity", "damping_alpha",
                  # *Energy Output inside an explicit step (bool): the driver keeps an energy balance of the run
                  "energy_output")

    def __init_subclass__(cls, **kwargs):
        super().__init_subclass__(**kwargs)
        missing = [m for m in REQUIRED if not callable(getattr(cls, m, None))]
        if missing:
            raise TypeError(f"{cls.__name__} does not implement the reader interface: missing {missing}")

    def __init__(self, file_name: str):
        raise NotImplementedError("InpInfoBase is an interface; use reader.InpInfo")
