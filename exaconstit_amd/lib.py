"""ctypes binding of libexaconstit_hip.so (the C ABI of include/exaconstit_hip.h).

No CPU fallback: if the library is missing this module raises at import; if no GPU is present exa_create fails.
Device memory is passed as raw pointers (torch tensors' data_ptr() in the tests/bench — PyTorch is only the allocator).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EXA_LIB") or os.path.join(_HERE, "libexaconstit_hip.so")   # EXA_LIB: a timing variant built by `make variant` (experiments only)

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} not found: build it with `make -C exaconstit_amd/csrc` (or __graft_entry__.build()); "
        "there is no CPU fallback for the product path")

# PyTorch bundles its own HIP runtime (soname libamdhip64.so.7).  Two HIP runtimes in one process do not share
# devices, so when torch is the allocator it must be loaded FIRST: the dynamic loader then resolves this library's
# NEEDED libamdhip64.so.7 to the copy torch already mapped.
try:
    import torch  # noqa: F401
except ImportError:  # stand-alone use (C++ driver, plain ctypes): the system ROCm runtime is used
    torch = None

_lib = C.CDLL(LIB_PATH)

EXA_FCC_VOCE, EXA_FCC_VOCE_NL, EXA_BCC_VOCE, EXA_BCC_VOCE_NL, EXA_FCC_KMDD, EXA_BCC_KMDD = range(6)
EXA_ASSEMBLY_PA, EXA_ASSEMBLY_EA = 0, 1
EXA_INTEG_FULL, EXA_INTEG_BBAR = 0, 1

dptr = C.c_void_p


class ExaConfig(C.Structure):
    _fields_ = [("model", C.c_int), ("nprops", C.c_int), ("props", C.POINTER(C.c_double)), ("temp_k", C.c_double),
                ("order", C.c_int), ("nelems", C.c_int), ("assembly", C.c_int), ("integ", C.c_int), ("device", C.c_int)]


def _sig(name, restype, *argtypes):
    f = getattr(_lib, name)
    f.restype = restype
    f.argtypes = list(argtypes)
    return f


# every symbol the header declares (tests check the list against include/exaconstit_hip.h)
exa_create = _sig("exa_create", C.c_void_p, C.POINTER(ExaConfig), C.POINTER(C.c_int))
exa_destroy = _sig("exa_destroy", None, C.c_void_p)
exa_last_error = _sig("exa_last_error", C.c_char_p, C.c_void_p)
exa_build_id = _sig("exa_build_id", C.c_char_p)
exa_kernel_build_id = _sig("exa_kernel_build_id", C.c_char_p)
exa_num_state_vars = _sig("exa_num_state_vars", C.c_int, C.c_void_p)
exa_nodes_per_elem = _sig("exa_nodes_per_elem", C.c_int, C.c_void_p)
exa_qpts_per_elem = _sig("exa_qpts_per_elem", C.c_int, C.c_void_p)
exa_shape_table = _sig("exa_shape_table", C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double))
exa_create_geom = _sig("exa_create_geom", C.c_void_p, C.POINTER(ExaConfig), C.c_int, C.POINTER(C.c_int))
exa_element_geometry = _sig("exa_element_geometry", C.c_int, C.c_void_p)
exa_ref_elem_tables = _sig("exa_ref_elem_tables", C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double))
EXA_GEOM_HEX, EXA_GEOM_TET = 0, 1
exa_set_quadrature_layout = _sig("exa_set_quadrature_layout", C.c_int, C.c_void_p, C.c_int)
exa_get_quadrature_layout = _sig("exa_get_quadrature_layout", C.c_int, C.c_void_p)
exa_set_aos_staging = _sig("exa_set_aos_staging", C.c_int, C.c_void_p, C.c_int)
exa_get_aos_staging = _sig("exa_get_aos_staging", C.c_int, C.c_void_p)
exa_qf_size = _sig("exa_qf_size", C.c_int64, C.c_void_p, C.c_int)
EXA_QLAYOUT_AOS, EXA_QLAYOUT_EB64 = 0, 1
EXA_OK, EXA_ERR_ARG, EXA_ERR_HIP, EXA_ERR_STATE, EXA_ERR_UNSUPPORTED = 0, -1, -2, -3, -4
exa_init_state = _sig("exa_init_state", C.c_int, C.c_void_p, dptr, dptr, C.c_void_p)
exa_state_normalize = _sig("exa_state_normalize", C.c_int, C.c_void_p, dptr, C.c_void_p)
exa_qf_pack = _sig("exa_qf_pack", C.c_int, C.c_void_p, C.c_int, dptr, dptr, dptr, C.c_void_p)
exa_qf_unpack = _sig("exa_qf_unpack", C.c_int, C.c_void_p, C.c_int, dptr, dptr, dptr, C.c_void_p)
exa_model_setup = _sig("exa_model_setup", C.c_int, C.c_void_p, C.c_double, dptr, dptr, dptr, dptr, dptr, dptr, dptr, C.c_void_p)
exa_model_setup_checked = _sig("exa_model_setup_checked", C.c_int, C.c_void_p, C.c_double, dptr, dptr, dptr, dptr, dptr, dptr, dptr, C.c_void_p)
exa_model_setup_lvec_records = _sig("exa_model_setup_lvec_records", C.c_int, C.c_void_p, C.c_double, dptr, dptr, dptr, dptr, dptr, dptr, dptr, C.c_void_p)
exa_model_setup_lvec = _sig("exa_model_setup_lvec", C.c_int, C.c_void_p, C.c_double, dptr, dptr, dptr, dptr, dptr, dptr, dptr, dptr, C.c_void_p)
exa_set_newton_cap = _sig("exa_set_newton_cap", C.c_int, C.c_void_p, C.c_int)
exa_selftest_km_math = _sig("exa_selftest_km_math", C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p)
exa_selftest_rot_math = _sig("exa_selftest_rot_math", C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p)
exa_set_newton_caps = _sig("exa_set_newton_caps", C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int)
exa_model_tail_count = _sig("exa_model_tail_count", C.c_int, C.c_void_p, C.c_void_p)
exa_model_record_launches = _sig("exa_model_record_launches", C.c_int, C.c_void_p, C.POINTER(C.c_longlong))
exa_set_newton_cap_auto = _sig("exa_set_newton_cap_auto", C.c_int, C.c_void_p, C.c_int, C.c_double)
exa_get_newton_cap = _sig("exa_get_newton_cap", C.c_int, C.c_void_p)
exa_set_lean_state = _sig("exa_set_lean_state", C.c_int, C.c_void_p, C.c_int)
exa_get_lean_state = _sig("exa_get_lean_state", C.c_int, C.c_void_p)
exa_slip_rates_from_state = _sig("exa_slip_rates_from_state", C.c_int, C.c_void_p, dptr, C.c_void_p)
exa_model_nfev_hist = _sig("exa_model_nfev_hist", C.c_int, C.c_void_p, dptr, C.POINTER(C.c_int), C.c_void_p)
exa_model_status = _sig("exa_model_status", C.c_int, C.c_void_p, C.c_void_p)
exa_calc_dp = _sig("exa_calc_dp", C.c_int, C.c_void_p, dptr, dptr, C.c_void_p)
exa_jacobians = _sig("exa_jacobians", C.c_int, C.c_void_p, dptr, dptr, C.c_void_p)
exa_jacobians_from_geom = _sig("exa_jacobians_from_geom", C.c_int, C.c_void_p, dptr, dptr, C.c_void_p)
exa_grad_calc = _sig("exa_grad_calc", C.c_int, C.c_void_p, dptr, dptr, dptr, C.c_void_p)
exa_residual_setup = _sig("exa_residual_setup", C.c_int, C.c_void_p, dptr, dptr, C.c_void_p)
exa_residual_apply = _sig("exa_residual_apply", C.c_int, C.c_void_p, dptr, C.c_void_p)
exa_grad_setup = _sig("exa_grad_setup", C.c_int, C.c_void_p, C.c_double, dptr, dptr, C.c_void_p)
exa_grad_apply = _sig("exa_grad_apply", C.c_int, C.c_void_p, dptr, dptr, C.c_void_p)
exa_grad_diagonal = _sig("exa_grad_diagonal", C.c_int, C.c_void_p, dptr, C.c_void_p)
exa_grad_get_ea = _sig("exa_grad_get_ea", C.c_int, C.c_void_p, dptr, C.c_void_p)
exa_set_connectivity = _sig("exa_set_connectivity", C.c_int, C.c_void_p, dptr, C.c_int)
exa_restrict = _sig("exa_restrict", C.c_int, C.c_void_p, dptr, dptr, C.c_void_p)
exa_restrict_transpose_add = _sig("exa_restrict_transpose_add", C.c_int, C.c_void_p, dptr, dptr, C.c_void_p)
exa_grad_apply_lvec = _sig("exa_grad_apply_lvec", C.c_int, C.c_void_p, dptr, dptr, dptr, C.c_void_p)
exa_set_tangent_form = _sig("exa_set_tangent_form", C.c_int, C.c_void_p, C.c_int)
exa_set_deterministic = _sig("exa_set_deterministic", C.c_int, C.c_void_p, C.c_int)
exa_grad_tangent_defect = _sig("exa_grad_tangent_defect", C.c_int, C.c_void_p, dptr, C.POINTER(C.c_double), C.c_void_p)
EXA_TANGENT_FULL, EXA_TANGENT_DEV5_BULK, EXA_TANGENT_DEV5_BULK_GEO = 0, 1, 2
exa_set_ea_matrix_free = _sig("exa_set_ea_matrix_free", C.c_int, C.c_void_p, C.c_int)
exa_grad_set_coords = _sig("exa_grad_set_coords", C.c_int, C.c_void_p, dptr)
exa_residual_lvec = _sig("exa_residual_lvec", C.c_int, C.c_void_p, dptr, dptr, dptr, C.c_void_p)
exa_vol_avg = _sig("exa_vol_avg", C.c_int, C.c_void_p, dptr, dptr, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_void_p)
exa_element_fields = _sig("exa_element_fields", C.c_int, C.c_void_p, dptr, dptr, dptr, dptr, dptr, C.c_void_p)
exa_lattice_strains = _sig("exa_lattice_strains", C.c_int, C.c_void_p, dptr, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double),
                           C.c_double, dptr, C.c_void_p)
exa_cubic_fiber_axes = _sig("exa_cubic_fiber_axes", C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int)
EXA_LATTICE_MAX_HKL = 16
exa_grain_sums = _sig("exa_grain_sums", C.c_int, C.c_void_p, C.c_int, dptr, C.POINTER(C.c_int32), C.c_void_p, C.c_int, dptr, dptr, dptr, C.c_void_p)
exa_grain_plan = _sig("exa_grain_plan", C.c_int, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64))
EXA_GRAIN_NSUMS = 39
exa_texture_weights = _sig("exa_texture_weights", C.c_int, C.c_void_p, dptr, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_double),
                           C.c_double, C.c_int, dptr, C.c_void_p)
exa_texture_volume_max = _sig("exa_texture_volume_max", C.c_int, C.c_void_p, dptr, dptr, C.c_void_p)
exa_texture_quantum_log2 = _sig("exa_texture_quantum_log2", C.c_int, C.c_double, C.c_int64)
exa_texture_grid = _sig("exa_texture_grid", C.c_int, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_int))
exa_texture_bin = _sig("exa_texture_bin", C.c_int, C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_int))
EXA_TEXTURE_MAX_HKL, EXA_TEXTURE_MAX_DIRS = 16, 3
TEXTURE_HKL = ((1, 1, 1), (2, 0, 0), (2, 2, 0))     # the defaults of Visualizations.texture_hkl and texture_ipf_dirs
TEXTURE_IPF_DIRS = ((0, 0, 1),)
# columns of the exa_element_fields rows (include/exaconstit_hip.h)
EXA_NFIELDS = 37
ELEMENT_FIELDS = {"ElementVolume": (0, 1), "ElemCentroid": (1, 3), "Stress": (4, 6), "VonMisesStress": (10, 1), "HydrostaticStress": (11, 1),
                  "DpEff": (12, 1), "EffPlasticStrain": (13, 1), "Hardness": (14, 1), "ShearRate": (15, 12), "LatticeOrientation": (27, 4),
                  "XtalElasticStrain": (31, 6)}

MODEL_IDS = {("fcc", "powervoce"): EXA_FCC_VOCE, ("fcc", "powervocenl"): EXA_FCC_VOCE_NL, ("bcc", "powervoce"): EXA_BCC_VOCE,
             ("bcc", "powervocenl"): EXA_BCC_VOCE_NL, ("fcc", "mtsdd"): EXA_FCC_KMDD, ("bcc", "mtsdd"): EXA_BCC_KMDD}


class Context:
    """Owns one exa_ctx.  Mirrors how the reference's operator owns its model + integrator (mechanics_operator.cpp:49-225)."""

    def __init__(self, model, props, temp_k, order, nelems, assembly=EXA_ASSEMBLY_PA, integ=EXA_INTEG_FULL, device=-1, geometry=EXA_GEOM_HEX):
        import numpy as np
        self._props = np.ascontiguousarray(props, dtype=np.float64)
        cfg = ExaConfig(model, len(self._props), self._props.ctypes.data_as(C.POINTER(C.c_double)), float(temp_k),
                        order, nelems, assembly, integ, device)
        err = C.c_int(0)
        self.h = exa_create(C.byref(cfg), C.byref(err)) if geometry == EXA_GEOM_HEX else exa_create_geom(C.byref(cfg), geometry, C.byref(err))
        if not self.h:
            raise RuntimeError(f"exa_create failed with code {err.value} (is a HIP device present and the model/props valid?)")
        self.n = exa_nodes_per_elem(self.h)
        self.Q = exa_qpts_per_elem(self.h)
        self.E = nelems
        self.nstatev = exa_num_state_vars(self.h)

    def check(self, rc, what=""):
        if rc < 0:
            raise RuntimeError(f"{what} failed ({rc}): {exa_last_error(self.h).decode()}")
        return rc

    def shape_table(self):
        import numpy as np
        G = np.zeros(self.n * 3 * self.Q)
        W = np.zeros(self.Q)
        self.check(exa_shape_table(self.h, G.ctypes.data_as(C.POINTER(C.c_double)), W.ctypes.data_as(C.POINTER(C.c_double))))
        return G, W

    def close(self):
        if self.h:
            exa_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ref_elem_tables(geometry, order):
    """Reference-element tables of (geometry, order), host only: G (n,3,Q) flat, W (Q), N (n,Q) flat shape values."""
    import numpy as np
    rc = exa_ref_elem_tables(geometry, order, None, None, None)
    if rc < 0:
        raise ValueError(f"no reference element for geometry {geometry}, order {order}")
    n, Q = rc // 1000, rc % 1000
    G, W, N = np.zeros(n * 3 * Q), np.zeros(Q), np.zeros(n * Q)
    f = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    exa_ref_elem_tables(geometry, order, f(G), f(W), f(N))
    return G, W, N


# ---- stand-alone driver (include/exaconstit_driver.h) ---------------------------------------------------
class ExaSynthConfig(C.Structure):
    _fields_ = [("N", C.c_int), ("bcc", C.c_int), ("slip", C.c_int), ("nprops", C.c_int), ("props", C.POINTER(C.c_double)),
                ("temp_k", C.c_double), ("quats", C.POINTER(C.c_double)), ("assembly", C.c_int), ("nrls", C.c_int), ("jacobi", C.c_int),
                ("newton_iter", C.c_int), ("newton_rel", C.c_double), ("newton_abs", C.c_double),
                ("krylov_iter", C.c_int), ("krylov_rel", C.c_double), ("krylov_abs", C.c_double),
                ("nsteps", C.c_int), ("dts", C.POINTER(C.c_double)), ("vz", C.c_double), ("order", C.c_int), ("bbar", C.c_int),
                ("nrev", C.c_int), ("rev_steps", C.POINTER(C.c_int))]


exa_rccl_unique_id = _sig("exa_rccl_unique_id", C.c_int, C.c_void_p)
exa_comm_unique_id = _sig("exa_comm_unique_id", C.c_int, C.c_void_p, C.c_int)
exa_device_identity = _sig("exa_device_identity", C.c_int, C.c_char_p, C.c_int)
exa_driver_comm_info = _sig("exa_driver_comm_info", C.c_int, C.c_void_p, C.POINTER(C.c_int))
exa_loopback_group_create = _sig("exa_loopback_group_create", C.c_int, C.c_int, C.c_void_p)
exa_loopback_group_destroy = _sig("exa_loopback_group_destroy", None, C.c_void_p)
exa_driver_comm_details = _sig("exa_driver_comm_details", C.c_int, C.c_void_p, C.POINTER(C.c_int64))
exa_driver_comm_probe = _sig("exa_driver_comm_probe", C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_int)
exa_comm_rank_fold = _sig("exa_comm_rank_fold", C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double))
exa_operator_routes_query = _sig("exa_operator_routes_query", C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.c_int)
exa_driver_create = _sig("exa_driver_create", C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_int)
exa_driver_create_synthetic = _sig("exa_driver_create_synthetic", C.c_void_p, C.POINTER(ExaSynthConfig), C.c_int, C.c_int, C.c_void_p, C.c_char_p, C.c_int)
exa_driver_destroy = _sig("exa_driver_destroy", None, C.c_void_p)
exa_driver_num_steps = _sig("exa_driver_num_steps", C.c_int, C.c_void_p)
exa_driver_local_qpts = _sig("exa_driver_local_qpts", C.c_int64, C.c_void_p)
exa_driver_mesh_info = _sig("exa_driver_mesh_info", C.c_int, C.c_void_p, C.POINTER(C.c_int64))
ACTION_ROUTES = ("hex", "tet_fused", "generic_evector", "generic_ea_lvec")
exa_driver_local_dofs = _sig("exa_driver_local_dofs", C.c_int64, C.c_void_p)
exa_driver_step = _sig("exa_driver_step", C.c_int, C.c_void_p, C.c_int, C.c_char_p, C.c_int)
exa_driver_step_nocommit = _sig("exa_driver_step_nocommit", C.c_int, C.c_void_p, C.c_int, C.c_char_p, C.c_int)
exa_driver_commit_step = _sig("exa_driver_commit_step", C.c_int, C.c_void_p, C.c_char_p, C.c_int)
exa_driver_run = _sig("exa_driver_run", C.c_int, C.c_void_p, C.c_char_p, C.c_int)
exa_driver_get_avgs = _sig("exa_driver_get_avgs", C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_int)
exa_driver_get_stats = _sig("exa_driver_get_stats", C.c_int, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int)
exa_driver_get_timers = _sig("exa_driver_get_timers", None, C.c_void_p, C.POINTER(C.c_double))
exa_driver_reset_timers = _sig("exa_driver_reset_timers", None, C.c_void_p)
exa_driver_nfev_hist = _sig("exa_driver_nfev_hist", C.c_int, C.c_void_p, C.POINTER(C.c_int), C.c_char_p, C.c_int)
exa_driver_get_qf_component = _sig("exa_driver_get_qf_component", C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_char_p, C.c_int)
exa_driver_nfev_hist_of = _sig("exa_driver_nfev_hist_of", C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_char_p, C.c_int)
exa_driver_get_diagnostics = _sig("exa_driver_get_diagnostics", None, C.c_void_p, C.POINTER(C.c_int64))
exa_driver_get_rate_launches = _sig("exa_driver_get_rate_launches", C.c_int64, C.c_void_p)
exa_driver_get_record_launches = _sig("exa_driver_get_record_launches", None, C.c_void_p, C.POINTER(C.c_int64))
exa_driver_get_field_launches = _sig("exa_driver_get_field_launches", C.c_int64, C.c_void_p)
exa_rccl_microbench = _sig("exa_rccl_microbench", C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_char_p, C.c_int)
exa_bootstrap_env = _sig("exa_bootstrap_env", C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int))
exa_bootstrap_reply_fn = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p)
exa_bootstrap_gather_reply = _sig("exa_bootstrap_gather_reply", C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, exa_bootstrap_reply_fn, C.c_void_p,
                                  C.c_double, C.c_char_p, C.c_int)
exa_transport_from_identities = _sig("exa_transport_from_identities", C.c_int, C.c_void_p, C.c_int, C.c_char_p, C.c_int)
exa_bootstrap_bcast = _sig("exa_bootstrap_bcast", C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_char_p, C.c_int)
exa_bootstrap = _sig("exa_bootstrap", C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_char_p, C.c_int)
exa_driver_get_pcg_reduction = _sig("exa_driver_get_pcg_reduction", None, C.c_void_p, C.POINTER(C.c_double))
exa_driver_bench_prepare = _sig("exa_driver_bench_prepare", C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_double, C.c_char_p, C.c_int)
exa_driver_bench_model = _sig("exa_driver_bench_model", C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_char_p, C.c_int)
exa_driver_bench_adapter_route = _sig("exa_driver_bench_adapter_route", C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_char_p, C.c_int)
exa_driver_bench_pcg = _sig("exa_driver_bench_pcg", C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_char_p, C.c_int)
exa_choose_newton_cap = _sig("exa_choose_newton_cap", C.c_int, C.POINTER(C.c_int), C.c_double)
exa_choose_newton_caps = _sig("exa_choose_newton_caps", C.c_int, C.POINTER(C.c_int), C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_int))
exa_options_query = _sig("exa_options_query", C.c_int, C.c_char_p, C.POINTER(C.c_double), C.c_char_p, C.c_int)
exa_options_query_vis = _sig("exa_options_query_vis", C.c_int, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_int,
                             C.c_char_p, C.c_int)
exa_vtu_selftest = _sig("exa_vtu_selftest", C.c_int, C.c_char_p, C.POINTER(C.c_double), C.c_int, C.c_char_p, C.c_int)
exa_driver_element_fields = _sig("exa_driver_element_fields", C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                                 C.c_char_p, C.c_int)
exa_driver_lattice_strains = _sig("exa_driver_lattice_strains", C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_double,
                                  C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_char_p, C.c_int)
exa_options_query_lightup = _sig("exa_options_query_lightup", C.c_int, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                 C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int)
exa_driver_grain_averages = _sig("exa_driver_grain_averages", C.c_int, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int64, C.c_char_p, C.c_int)
exa_driver_set_grains = _sig("exa_driver_set_grains", C.c_int, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int, C.c_int64, C.c_char_p, C.c_int)
exa_driver_create_restart = _sig("exa_driver_create_restart", C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_int)
exa_driver_save_checkpoint = _sig("exa_driver_save_checkpoint", C.c_int, C.c_void_p, C.c_char_p, C.c_char_p, C.c_int)
exa_driver_load_checkpoint = _sig("exa_driver_load_checkpoint", C.c_int, C.c_void_p, C.c_char_p, C.c_char_p, C.c_int)
exa_checkpoint_info = _sig("exa_checkpoint_info", C.c_int, C.c_char_p, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_char_p, C.POINTER(C.c_uint64),
                           C.c_int, C.c_char_p, C.c_int)
exa_options_query_checkpoint = _sig("exa_options_query_checkpoint", C.c_int, C.c_char_p, C.POINTER(C.c_int), C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_char_p, C.c_int)
exa_partition_query_nodes = _sig("exa_partition_query_nodes", C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_void_p)
exa_mesh_partition_query_nodes = _sig("exa_mesh_partition_query_nodes", C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_void_p, C.c_char_p, C.c_int)
exa_options_query_grains = _sig("exa_options_query_grains", C.c_int, C.c_char_p, C.POINTER(C.c_int), C.c_char_p, C.c_int, C.c_char_p, C.c_int)
exa_grain_avgs_write = _sig("exa_grain_avgs_write", C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_char_p, C.c_int)
EXA_GRAIN_NVALS = 45
# value columns of exa_driver_grain_averages and of the grain_avgs files after the grain id (include/exaconstit_driver.h): name -> (first, count)
GRAIN_COLUMNS = {"n_elements": (0, 1), "volume": (1, 1), "volume_fraction": (2, 1), "Stress": (3, 6), "VonMisesStress": (9, 1), "HydrostaticStress": (10, 1),
                 "ElasticStrainSample": (11, 6), "XtalElasticStrain": (17, 6), "EffPlasticStrain": (23, 1), "DpEff": (24, 1), "Hardness": (25, 1),
                 "ShearRate": (26, 12), "LatticeOrientation": (38, 4), "MisorientationMean": (42, 1), "MisorientationMax": (43, 1), "GrainRotation": (44, 1)}


def grain_dict(ids, vals):
    """{"grain_id": (n,), column name: (n,) or (n, count)} from grain ids and (n, EXA_GRAIN_NVALS) values"""
    import numpy as np
    out = {"grain_id": np.asarray(ids, dtype=np.int64)}
    for k, (c0, n) in GRAIN_COLUMNS.items():
        out[k] = vals[:, c0] if n == 1 else vals[:, c0:c0 + n].copy()
    out["n_elements"] = np.rint(out["n_elements"]).astype(np.int64)
    return out


def write_grain_avgs(path, ids, vals):
    """the driver's grain_avgs file writer (host only): header line, then one row per grain"""
    import numpy as np
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    vals = np.ascontiguousarray(vals, dtype=np.float64).reshape(len(ids), EXA_GRAIN_NVALS)
    err = C.create_string_buffer(512)
    if exa_grain_avgs_write(str(path).encode(), len(ids), ids.ctypes.data_as(C.POINTER(C.c_int32)), vals.ctypes.data_as(C.POINTER(C.c_double)), err, 512) != 0:
        raise RuntimeError(err.value.decode())


def read_grain_avgs(path):
    """a grain_avgs file as the dict of Driver.grain_averages()"""
    import numpy as np
    a = np.loadtxt(path, ndmin=2).reshape(-1, 1 + EXA_GRAIN_NVALS)
    return grain_dict(np.rint(a[:, 0]).astype(np.int64), a[:, 1:])


# intragranular misorientation and lattice curvature (include/exaconstit_hip.h)
exa_curvature_nodal = _sig("exa_curvature_nodal", C.c_int, C.c_void_p, dptr, C.c_void_p, C.c_int, dptr, dptr, dptr, C.c_void_p)
exa_curvature_elements = _sig("exa_curvature_elements", C.c_int, C.c_void_p, dptr, C.c_void_p, C.c_int, dptr, dptr, dptr, dptr, C.c_double, dptr, C.c_void_p)
exa_curvature_summary = _sig("exa_curvature_summary", C.c_int, C.c_void_p, dptr, dptr, dptr, C.c_void_p)
exa_curvature_sizes = _sig("exa_curvature_sizes", C.c_int, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int))
exa_driver_lattice_curvature = _sig("exa_driver_lattice_curvature", C.c_int, C.c_void_p, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                                    C.POINTER(C.c_double), C.c_char_p, C.c_int)
exa_options_query_lattice_curvature = _sig("exa_options_query_lattice_curvature", C.c_int, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_char_p, C.c_int,
                                           C.c_char_p, C.c_int)
EXA_NCURV = 16
# columns of the rows of exa_curvature_elements / exa_driver_lattice_curvature: name -> (first, count)
CURVATURE_COLUMNS = {"RotationVector": (0, 3), "GROD": (3, 1), "KAM": (4, 1), "LatticeCurvature": (5, 9), "NyeNorm": (14, 1), "GNDDensity": (15, 1)}
# the values of "summary" (Driver.lattice_curvature) and, after step and time, the columns of the lattice_curvature file
CURVATURE_SUMMARY = ("GROD_mean", "GROD_max", "KAM_mean", "KAM_max", "GNDDensity_mean", "GNDDensity_max")


def curvature_sizes(E):
    """(doubles of work_dev for E elements, planes of nodal_dev) of exa_curvature_nodal (host only)"""
    w, pl = C.c_int64(), C.c_int()
    if exa_curvature_sizes(int(E), C.byref(w), C.byref(pl)) != 0:
        raise ValueError(f"E = {E} must not be negative")
    return w.value, pl.value


def options_lattice_curvature(path):
    """lattice-curvature keys of the Visualizations table: dict(enabled, burgers, fname)"""
    en, b = C.c_int(), C.c_double()
    f = C.create_string_buffer(4096)
    err = C.create_string_buffer(512)
    if exa_options_query_lattice_curvature(path.encode(), C.byref(en), C.byref(b), f, 4096, err, 512) != 0:
        raise RuntimeError(err.value.decode())
    return dict(enabled=bool(en.value), burgers=b.value, fname=f.value.decode())


def read_lattice_curvature(path):
    """a lattice_curvature file of the driver: dict(step (n,) int64, time (n,), and (n,) per CURVATURE_SUMMARY name), one entry per written step"""
    import numpy as np
    with open(path) as f:
        head = f.readline().split()
    names = ["step", "time", "grod_mean_deg", "grod_max_deg", "kam_mean_deg", "kam_max_deg", "gnd_density_mean", "gnd_density_max"]
    if head != ["#"] + names:
        raise ValueError(f"{path}: not a lattice_curvature file (header {head})")
    a = np.loadtxt(path, ndmin=2).reshape(-1, len(names))
    out = {"step": np.rint(a[:, 0]).astype(np.int64), "time": a[:, 1].copy()}
    for k, nm in enumerate(CURVATURE_SUMMARY):
        out[nm] = a[:, 2 + k].copy()
    return out


# slip-system activity and the Fatemi-Socie fatigue indicator parameter (include/exaconstit_hip.h)
exa_slip_activity_sizes = _sig("exa_slip_activity_sizes", C.c_int, C.c_int64, C.POINTER(C.c_int64))
exa_slip_accumulate = _sig("exa_slip_accumulate", C.c_int, C.c_void_p, dptr, C.POINTER(C.c_double), C.c_double, C.c_int, dptr, C.c_void_p)
exa_fip_rows = _sig("exa_fip_rows", C.c_int, C.c_void_p, dptr, C.c_double, C.c_double, dptr, C.c_void_p)
exa_fip_summary = _sig("exa_fip_summary", C.c_int, C.c_void_p, dptr, dptr, dptr, dptr, C.c_void_p)
exa_slip_plane_normals = _sig("exa_slip_plane_normals", C.c_int, C.c_int, C.POINTER(C.c_double))
exa_fatigue_scratch_bytes = _sig("exa_fatigue_scratch_bytes", C.c_int, C.POINTER(C.c_int))
exa_driver_enable_slip_activity = _sig("exa_driver_enable_slip_activity", C.c_int, C.c_void_p, C.c_char_p, C.c_int)
exa_driver_reset_fatigue_window = _sig("exa_driver_reset_fatigue_window", C.c_int, C.c_void_p, C.c_char_p, C.c_int)
exa_driver_slip_activity = _sig("exa_driver_slip_activity", C.c_int, C.c_void_p, C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int64,
                                C.POINTER(C.c_int64), C.c_char_p, C.c_int)
exa_options_query_fatigue = _sig("exa_options_query_fatigue", C.c_int, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_char_p, C.c_int, C.c_char_p, C.c_int)
exa_fatigue_write = _sig("exa_fatigue_write", C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_double), C.c_int, C.c_char_p, C.c_int)
exa_fatigue_grains_write = _sig("exa_fatigue_grains_write", C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_char_p, C.c_int)
EXA_NSLIPACC, EXA_NFIP = 60, 6
# planes of the accumulators (12 slip systems each) and columns of the rows of exa_fip_rows, in their stored order
SLIP_ACC_PLANES = ("SlipAccumulated", "SlipAbsolute", "SlipMin", "SlipMax", "NormalStressMax")
FIP_COLUMNS = ("FIP", "FIPSystem", "ShearRange", "NormalStressMax", "AccumulatedSlip", "NetSlipMax")
# the values of "summary" (Driver.slip_activity); the fatigue file holds step, time, window_start_step and then the six after "volume"
FATIGUE_SUMMARY = ("volume", "FIP_mean", "FIP_max", "FIP_max_element", "AccumulatedSlip_mean", "AccumulatedSlip_max", "ShearRange_max", "window_start_step")
_FATIGUE_HEAD = ["step", "time", "window_start_step", "fip_mean", "fip_max", "fip_max_element", "accumulated_slip_mean", "accumulated_slip_max", "shear_range_max"]


def slip_activity_sizes(E):
    """doubles of the accumulators of E elements: 60 planes of E rounded up to 64 (host only)"""
    n = C.c_int64()
    if exa_slip_activity_sizes(int(E), C.byref(n)) != 0:
        raise ValueError(f"E = {E} must not be negative")
    return n.value


def slip_plane_normals(model):
    """(12, 3) unit slip-plane normals in the crystal frame of the model's systems, in the order of the slip rates (host only)"""
    import numpy as np
    out = np.zeros((12, 3))
    if exa_slip_plane_normals(int(model), out.ctypes.data_as(C.POINTER(C.c_double))) != 0:
        raise ValueError(f"model {model} has no slip-plane table")
    return out


def fatigue_scratch_bytes():
    """private bytes per lane of k_slip_accumulate (plain, fused reset), k_fip_rows, k_fip_partial, k_fip_reduce in the loaded code object"""
    o = (C.c_int * 8)()
    if exa_fatigue_scratch_bytes(o) != 0:
        raise RuntimeError("exa_fatigue_scratch_bytes: no device")
    return list(o)[:5]


def options_fatigue(path):
    """fatigue keys of the Visualizations table: dict(enabled, k, sigma_y (0.0 when absent), cycle_steps, fname)"""
    i2, d2 = (C.c_int * 2)(), (C.c_double * 2)()
    f = C.create_string_buffer(4096)
    err = C.create_string_buffer(512)
    if exa_options_query_fatigue(path.encode(), i2, d2, f, 4096, err, 512) != 0:
        raise RuntimeError(err.value.decode())
    return dict(enabled=bool(i2[0]), cycle_steps=int(i2[1]), k=d2[0], sigma_y=d2[1], fname=f.value.decode())


def read_fatigue(path):
    """a fatigue file of the driver: dict(step, window_start_step, FIP_max_element (n,) int64; time and the other FATIGUE_SUMMARY names (n,)), one entry per evaluation"""
    import numpy as np
    with open(path) as f:
        head = f.readline().split()
    if head != ["#"] + _FATIGUE_HEAD:
        raise ValueError(f"{path}: not a fatigue file (header {head})")
    with open(path) as f:
        rows = [ln.split() for ln in f if ln.strip() and not ln.startswith("#")]
    if any(len(r) != len(_FATIGUE_HEAD) for r in rows):
        raise ValueError(f"{path}: a row does not hold {len(_FATIGUE_HEAD)} values")
    col = lambda k, t: np.array([t(r[k]) for r in rows], dtype=np.int64 if t is int else np.float64)
    out = {"step": col(0, int), "time": col(1, float), "window_start_step": col(2, int), "FIP_mean": col(3, float), "FIP_max": col(4, float),
           "FIP_max_element": col(5, int), "AccumulatedSlip_mean": col(6, float), "AccumulatedSlip_max": col(7, float), "ShearRange_max": col(8, float)}
    return out


def read_fatigue_grains(path):
    """a fatigue_grains file of the driver as the "grains" dict of Driver.slip_activity(): grain_id (n,) int64, volume, FIP_mean, FIP_max (n,)"""
    import numpy as np
    with open(path) as f:
        head = f.readline().split()
    if head != ["#", "grain_id", "volume", "fip_mean", "fip_max"]:
        raise ValueError(f"{path}: not a fatigue_grains file (header {head})")
    a = np.loadtxt(path, ndmin=2).reshape(-1, 4)
    return {"grain_id": np.rint(a[:, 0]).astype(np.int64), "volume": a[:, 1].copy(), "FIP_mean": a[:, 2].copy(), "FIP_max": a[:, 3].copy()}


exa_driver_pole_figures = _sig("exa_driver_pole_figures", C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_double), C.c_double,
                               C.POINTER(C.c_double), C.c_char_p, C.c_int)
exa_options_query_texture = _sig("exa_options_query_texture", C.c_int, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                 C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_char_p, C.c_int, C.c_char_p, C.c_int)


def texture_grid(res_deg):
    """(n_alpha, n_beta) of the texture grid of resolution res_deg (exa_texture_grid); ValueError unless res_deg divides 90 and lies in [2, 30]"""
    na, nb = C.c_int(), C.c_int()
    if exa_texture_grid(float(res_deg), C.byref(na), C.byref(nb)) != 0:
        raise ValueError(f"res_deg = {res_deg} must divide 90 and lie in [2, 30]")
    return na.value, nb.value


def texture_bin(p, res_deg):
    """(ring i, sector k) of the direction p on the texture grid - the kernel's binning code (exa_texture_bin)"""
    v = (C.c_double * 3)(*[float(x) for x in p])
    i, k = C.c_int(), C.c_int()
    if exa_texture_bin(v, float(res_deg), C.byref(i), C.byref(k)) != 0:
        raise ValueError(f"res_deg = {res_deg} must divide 90 and lie in [2, 30]")
    return i.value, k.value


def texture_cells(res_deg):
    """alpha_edges (n_alpha + 1,), beta_edges (n_beta + 1,) in degrees and the solid angle (n_alpha,) of one bin of each ring:
    res (cos i res - cos (i + 1) res), res in radians (the n_alpha x n_beta bins sum to 2 pi)"""
    import numpy as np
    na, nb = texture_grid(res_deg)
    r = np.radians(res_deg)
    i = np.arange(na)
    return res_deg * np.arange(na + 1), res_deg * np.arange(nb + 1), r * (np.cos(i * r) - np.cos((i + 1) * r))


def texture_weights(ctx, fields_dev, hkl, ipf_dirs, res_deg, quantum_log2, out_dev, stream=None):
    """launch exa_texture_weights on the device rows fields_dev (pointer, [E][EXA_NFIELDS]) of the context ctx: the pole figures of the families
    hkl and the inverse pole figures of the directions ipf_dirs into the int64 counts out_dev (pointer, [H + D][n_alpha][n_beta]); does not synchronise"""
    import numpy as np
    hkl = [tuple(h) for h in hkl]
    axes = [cubic_fiber_axes(*h) for h in hkl]
    off = np.concatenate([[0], np.cumsum([len(a) for a in axes])]).astype(np.int32)
    ax = np.ascontiguousarray(np.concatenate(axes) if axes else np.zeros((1, 3)))
    d = np.ascontiguousarray(np.asarray(ipf_dirs, dtype=np.float64).reshape(-1, 3) if len(ipf_dirs) else np.zeros((1, 3)))
    ctx.check(exa_texture_weights(ctx.h, fields_dev, len(hkl), ax.ctypes.data_as(C.POINTER(C.c_double)), off.ctypes.data_as(C.POINTER(C.c_int)),
                                  len(ipf_dirs), d.ctypes.data_as(C.POINTER(C.c_double)), float(res_deg), int(quantum_log2), out_dev, stream),
              "exa_texture_weights")


def options_texture(path):
    """texture keys of the Visualizations table: dict(enabled, hkl (list of triples), ipf_dirs (list of unit triples), res_deg, fname)"""
    en, nh, nd = C.c_int(), C.c_int(), C.c_int()
    hkl = (C.c_int * 48)()
    dirs = (C.c_double * 9)()
    res = C.c_double()
    f = C.create_string_buffer(4096)
    err = C.create_string_buffer(512)
    if exa_options_query_texture(path.encode(), C.byref(en), C.byref(nh), hkl, C.byref(nd), dirs, C.byref(res), f, 4096, err, 512) != 0:
        raise RuntimeError(err.value.decode())
    return dict(enabled=bool(en.value), hkl=[tuple(hkl[3 * j:3 * j + 3]) for j in range(nh.value)],
                ipf_dirs=[tuple(dirs[3 * m:3 * m + 3]) for m in range(nd.value)], res_deg=res.value, fname=f.value.decode())


def read_texture(path):
    """a texture file of the driver: dict(step, time, res_deg, hkl (list of triples), ipf_dirs (list of triples), pf (H, n_alpha, n_beta),
    ipf (D, n_alpha, n_beta))"""
    import numpy as np
    lines = open(path).read().splitlines()
    h = lines[0].split()
    assert h[:3] == ["#", "texture", "step"], h
    kv = dict(zip(h[2::2], h[3::2]))
    na, nb = int(kv["n_alpha"]), int(kv["n_beta"])
    hkl, dirs, pf, ipf = [], [], [], []
    i = 1
    while i < len(lines):
        head = lines[i]
        block = np.array([[float(x) for x in ln.split()] for ln in lines[i + 1:i + 1 + na]]).reshape(na, nb)
        if head.startswith("# pole figure {"):
            hkl.append(tuple(int(x) for x in head[head.index("{") + 1:head.index("}")].split()))
            pf.append(block)
        elif head.startswith("# inverse pole figure ["):
            dirs.append(tuple(float(x) for x in head[head.index("[") + 1:head.index("]")].split()))
            ipf.append(block)
        else:
            raise ValueError(f"{path}: unexpected line {head!r}")
        i += 1 + na
    return dict(step=int(kv["step"]), time=float(kv["time"]), res_deg=float(kv["res_deg"]), hkl=hkl, ipf_dirs=dirs,
                pf=np.array(pf).reshape(len(pf), na, nb), ipf=np.array(ipf).reshape(len(ipf), na, nb))


exa_driver_write_fields = _sig("exa_driver_write_fields", C.c_int, C.c_void_p, C.c_char_p, C.c_int, C.c_double, C.c_char_p, C.c_int)
_dp = C.POINTER(C.c_double)
exa_driver_set_preconditioner = _sig("exa_driver_set_preconditioner", C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int)
exa_driver_mg_info = _sig("exa_driver_mg_info", C.c_int, C.c_void_p, _dp)
exa_driver_mg_setup = _sig("exa_driver_mg_setup", C.c_int, C.c_void_p, C.c_char_p, C.c_int)
exa_driver_mg_level_dofs = _sig("exa_driver_mg_level_dofs", C.c_int64, C.c_void_p, C.c_int)
exa_driver_mg_apply = _sig("exa_driver_mg_apply", C.c_int, C.c_void_p, C.c_int, _dp, _dp)
exa_driver_mg_diag = _sig("exa_driver_mg_diag", C.c_int, C.c_void_p, C.c_int, _dp)
exa_driver_mg_transfer = _sig("exa_driver_mg_transfer", C.c_int, C.c_void_p, C.c_int, C.c_int, _dp, _dp)
exa_driver_mg_stencil = _sig("exa_driver_mg_stencil", C.c_int, C.c_void_p, C.c_int, _dp)
exa_driver_precond_apply = _sig("exa_driver_precond_apply", C.c_int, C.c_void_p, _dp, _dp)
exa_options_query_solver = _sig("exa_options_query_solver", C.c_int, C.c_char_p, C.POINTER(C.c_int), C.c_char_p, C.c_int)
exa_mg_level_count = _sig("exa_mg_level_count", C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int)

exa_driver_set_periodic = _sig("exa_driver_set_periodic", C.c_int, C.c_void_p, _dp, C.c_char_p, C.c_int)
exa_driver_periodic_info = _sig("exa_driver_periodic_info", C.c_int, C.c_void_p, C.POINTER(C.c_int64), _dp)
exa_driver_get_nodal = _sig("exa_driver_get_nodal", C.c_int, C.c_void_p, C.c_int, _dp, C.c_char_p, C.c_int)
exa_periodic_sum_scratch_bytes = _sig("exa_periodic_sum_scratch_bytes", C.c_int)
exa_driver_set_mg_periodic = _sig("exa_driver_set_mg_periodic", C.c_int, C.c_void_p, C.c_int)
exa_mg_periodic_scratch_bytes = _sig("exa_mg_periodic_scratch_bytes", C.c_int, C.POINTER(C.c_int))
exa_driver_set_mg_p2 = _sig("exa_driver_set_mg_p2", C.c_int, C.c_void_p, C.c_int)
exa_driver_set_mg_bbar = _sig("exa_driver_set_mg_bbar", C.c_int, C.c_void_p, C.c_int)
exa_driver_mg_bbar = _sig("exa_driver_mg_bbar", C.c_int, C.c_void_p)
exa_options_query_mg_bbar = _sig("exa_options_query_mg_bbar", C.c_int, C.c_char_p, C.POINTER(C.c_int), C.c_char_p, C.c_int)
exa_mg_p2_bbar_scratch_bytes = _sig("exa_mg_p2_bbar_scratch_bytes", C.c_int, C.POINTER(C.c_int))
exa_driver_set_mg_p2_build = _sig("exa_driver_set_mg_p2_build", C.c_int, C.c_void_p, C.c_int)
exa_driver_mg_info_order = _sig("exa_driver_mg_info_order", C.c_int, C.c_void_p, C.POINTER(C.c_int))
exa_mg_level_count_order = _sig("exa_mg_level_count_order", C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int)
exa_options_query_mg_p2 = _sig("exa_options_query_mg_p2", C.c_int, C.c_char_p, C.POINTER(C.c_int), C.c_char_p, C.c_int)
exa_mg_p2_scratch_bytes = _sig("exa_mg_p2_scratch_bytes", C.c_int, C.POINTER(C.c_int))
exa_grad_mg_p2_build = _sig("exa_grad_mg_p2_build", C.c_int, C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
exa_driver_newton_info = _sig("exa_driver_newton_info", C.c_int, C.c_void_p, _dp)
exa_options_query_bcs = _sig("exa_options_query_bcs", C.c_int, C.c_char_p, C.POINTER(C.c_int), _dp, C.c_int, C.c_char_p, C.c_int)
exa_partition_query_periodic = _sig("exa_partition_query_periodic", C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
exa_driver_set_periodic_mixed = _sig("exa_driver_set_periodic_mixed", C.c_int, C.c_void_p, _dp, C.POINTER(C.c_int), C.c_char_p, C.c_int)
exa_driver_macro_info = _sig("exa_driver_macro_info", C.c_int, C.c_void_p, C.POINTER(C.c_int), _dp, _dp, _dp)
exa_periodic_mixed_scratch_bytes = _sig("exa_periodic_mixed_scratch_bytes", C.c_int, C.POINTER(C.c_int))
exa_options_query_periodic_free = _sig("exa_options_query_periodic_free", C.c_int, C.c_char_p, C.POINTER(C.c_int), C.c_char_p, C.c_int)
exa_partition_query_periodic_mixed = _sig("exa_partition_query_periodic_mixed", C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)

exa_driver_macro_tangent = _sig("exa_driver_macro_tangent", C.c_int, C.c_void_p, C.c_double, C.c_int, C.c_int, _dp, _dp, _dp, C.POINTER(C.c_int), C.c_char_p, C.c_int)
exa_driver_grad_apply_columns = _sig("exa_driver_grad_apply_columns", C.c_int, C.c_void_p, C.c_int, _dp, _dp, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_char_p, C.c_int)
exa_driver_pcg_solve = _sig("exa_driver_pcg_solve", C.c_int, C.c_void_p, C.c_int, _dp, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, _dp, C.POINTER(C.c_int),
                            C.POINTER(C.c_int), _dp, C.POINTER(C.c_int), _dp, C.c_char_p, C.c_int)
exa_driver_set_tangent_route = _sig("exa_driver_set_tangent_route", C.c_int, C.c_void_p, C.c_int, C.c_int)
exa_driver_set_krylov = _sig("exa_driver_set_krylov", C.c_int, C.c_void_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int)
exa_driver_krylov_info = _sig("exa_driver_krylov_info", C.c_int, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int64))
exa_driver_gmres_solve = _sig("exa_driver_gmres_solve", C.c_int, C.c_void_p, C.c_int, _dp, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, _dp, C.POINTER(C.c_int),
                              C.POINTER(C.c_int), _dp, _dp, C.c_char_p, C.c_int)
exa_gmres_ortho_probe = _sig("exa_gmres_ortho_probe", C.c_int, C.c_int64, C.c_int, _dp, _dp, _dp, C.c_double, C.c_int, _dp, _dp, _dp, C.POINTER(C.c_int), C.c_char_p, C.c_int)
exa_gmres_ortho_bench = _sig("exa_gmres_ortho_bench", C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, _dp, C.c_char_p, C.c_int)
exa_gmres_column_probe = _sig("exa_gmres_column_probe", C.c_int, C.c_int, _dp, C.c_double, C.c_double, _dp, C.POINTER(C.c_int), _dp)
exa_gmres_multidot_chunk = _sig("exa_gmres_multidot_chunk", C.c_int)
GMRES_MULTIDOT_CHUNK = int(exa_gmres_multidot_chunk())   # basis vectors per pass of the multi-dot kernel (krylov_info()["multidot_chunk"])
GMRES_ORTHO = {"ifneeded": 0, "always": 1, "never": 2, "mgs": 3}   # EXA_GMRES_ORTHO and the ortho argument of the probes


def gmres_ortho_probe(weight, V, w, flag=0.0, mode="ifneeded"):
    """The two bandwidth kernels of GMRES's Gram-Schmidt on any shape (one GPU): w (n) against the rows of V (k, n) in the product weighted by
    weight (n).  flag != 0: the kernels' gate is closed.  dict(h (k) the column of H, w_out (n), wnorm2 = |w_out|^2 from the partial sums of the
    subtraction kernel, passes: 0 with the gate closed, else 1 + second passes)"""
    import numpy as np
    V = np.ascontiguousarray(np.atleast_2d(V), dtype=np.float64)
    w = np.ascontiguousarray(w, dtype=np.float64)
    weight = np.ascontiguousarray(weight, dtype=np.float64)
    k, n = V.shape
    if w.shape != (n,) or weight.shape != (n,):
        raise ValueError("gmres_ortho_probe: weight and w have the length of V's rows")
    h, wo, n2 = np.zeros(k), np.zeros(n), np.zeros(1)
    ps = C.c_int(0)
    err = C.create_string_buffer(512)
    if exa_gmres_ortho_probe(n, k, weight.ctypes.data_as(_dp), V.ctypes.data_as(_dp), w.ctypes.data_as(_dp), float(flag), GMRES_ORTHO[mode], h.ctypes.data_as(_dp),
                             wo.ctypes.data_as(_dp), n2.ctypes.data_as(_dp), C.byref(ps), err, 512) != 0:
        raise RuntimeError(err.value.decode())
    return dict(h=h, w_out=wo, wnorm2=float(n2[0]), passes=int(ps.value))


def gmres_ortho_bench(n, col, mode="ifneeded", reps=20):
    """measurement hook of scripts/gmres_compare.py: ms per orthogonalisation and normalisation of column col (col + 1 basis vectors of n entries) on device buffers of the call's own"""
    ms = C.c_double(0.0)
    err = C.create_string_buffer(512)
    if exa_gmres_ortho_bench(int(n), int(col), GMRES_ORTHO[mode], int(reps), C.byref(ms), err, 512) != 0:
        raise RuntimeError(err.value.decode())
    return float(ms.value)


def gmres_column_probe(Hbar, beta, final_norm=0.0):
    """Host only: the small algebra of GMRES's scalar kernel on the (m + 1, m) Hessenberg matrix Hbar as Gram-Schmidt leaves it and the first residual
    norm beta.  dict(resid (m) the residual norm after each column, flags (m) what the solver decides after it with the bound final_norm (0 running,
    1 converged, -1 breakdown), y (m) the back-substitution over all columns, ok: False when it met a zero pivot (those y_i are 0))"""
    import numpy as np
    Hbar = np.asarray(Hbar, dtype=np.float64)
    m = Hbar.shape[1]
    if Hbar.shape != (m + 1, m):
        raise ValueError("gmres_column_probe: Hbar is (m + 1, m)")
    Hc = np.ascontiguousarray(Hbar.T)   # column i contiguous, leading dimension m + 1
    resid, y, fl = np.zeros(m), np.zeros(m), np.zeros(m, np.int32)
    rc = exa_gmres_column_probe(m, Hc.ctypes.data_as(_dp), float(beta), float(final_norm), resid.ctypes.data_as(_dp), fl.ctypes.data_as(C.POINTER(C.c_int)), y.ctypes.data_as(_dp))
    if rc < 0:
        raise ValueError("gmres_column_probe: 1 to 100 columns")
    return dict(resid=resid, flags=fl.astype(int), y=y, ok=bool(rc))
exa_macro_tangent_condense = _sig("exa_macro_tangent_condense", C.c_int, _dp, C.POINTER(C.c_int), _dp)
exa_options_macro_tangent = _sig("exa_options_macro_tangent", C.c_int, C.c_char_p, C.POINTER(C.c_int), _dp, C.c_char_p, C.c_int, C.c_char_p, C.c_int)
exa_tangent_scratch_bytes = _sig("exa_tangent_scratch_bytes", C.c_int, C.POINTER(C.c_int))
exa_grad_apply_lvec_cols = _sig("exa_grad_apply_lvec_cols", C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p)

PRECOND_KINDS = {"identity": 0, "jacobi": 1, "multigrid": 2}
NODAL_FIELDS = {"velocity": 0, "coords": 1, "coords_ref": 2}


def options_bcs(path):
    """[BCs] table of an options file: dict(periodic, vel_grad: (entries, 3, 3) essential_vel_grad of every boundary-condition entry)"""
    import numpy as np
    out = (C.c_int * 2)()
    err = C.create_string_buffer(512)
    if exa_options_query_bcs(path.encode(), out, None, 0, err, 512) != 0:
        raise RuntimeError(err.value.decode())
    vg = np.zeros((out[1], 3, 3))
    if exa_options_query_bcs(path.encode(), out, vg.ctypes.data_as(_dp), out[1], err, 512) != 0:
        raise RuntimeError(err.value.decode())
    return dict(periodic=bool(out[0]), vel_grad=vg)


def options_periodic_free(path):
    """[BCs] periodic_free of an options file: dict(mixed, free (3, 3) bool)"""
    import numpy as np
    out = (C.c_int * 10)()
    err = C.create_string_buffer(512)
    if exa_options_query_periodic_free(path.encode(), out, err, 512) != 0:
        raise RuntimeError(err.value.decode())
    return dict(mixed=bool(out[0]), free=np.array(out[1:10], dtype=bool).reshape(3, 3))


def partition_periodic_mixed(N, rank, nranks, order=1):
    """The tables of mixed loading of a rank's block of the generated mesh: dict(NN, weight (NN,), faces [3 arrays of local nodes on
    the top face of direction d], ctrl (4,) local ids of c_0 .. c_3 or -1, img_nodes, img_code, canon (NN,), nbr_dofs, groups: local group count)"""
    import numpy as np
    n = (C.c_int * 3)(*([int(N)] * 3 if isinstance(N, int) else [int(v) for v in N]))
    info = (C.c_int64 * 8)()
    exa_partition_query_periodic_mixed(n, rank, nranks, order, info, None, None, None, None, None, None, None)
    NN, nf, ni, shared = int(info[0]), [int(info[1 + d]) for d in range(3)], int(info[4]), int(info[6])
    w, face, ctrl = np.zeros(NN), np.zeros(max(sum(nf), 1), np.int32), np.zeros(4, np.int32)
    im, ic, canon, nd = np.zeros(max(ni, 1), np.int32), np.zeros(max(ni, 1), np.uint8), np.zeros(NN, np.int64), np.zeros(max(shared, 1), np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    exa_partition_query_periodic_mixed(n, rank, nranks, order, info, vp(w), vp(face), vp(ctrl), vp(im), vp(ic), vp(canon), vp(nd))
    off = np.concatenate([[0], np.cumsum(nf)])
    return dict(NN=NN, weight=w, faces=[face[off[d]:off[d + 1]].copy() for d in range(3)], ctrl=ctrl, img_nodes=im[:ni], img_code=ic[:ni], canon=canon,
                nbr_dofs=nd[:shared], groups=int(info[7]))


def partition_periodic(N, rank, nranks, order=1):
    """The periodic view of a rank's block of the generated N0 x N1 x N2 mesh: dict(canon (NN,) canonical id of every local node,
    weight (NN,) = 1 / holders of the canonical id, nbrs [(rank, dofs)], groups [local node indices of a canonical id with >= 2 local images;
    the first one is the representative], group_sizes {2: n, 4: n, 8: n})."""
    import numpy as np
    n = (C.c_int * 3)(*([int(N)] * 3 if isinstance(N, int) else [int(v) for v in N]))
    info = (C.c_int64 * 8)()
    exa_partition_query_periodic(n, rank, nranks, order, info, None, None, None, None, None, None, None)
    NN, nnb, shared, ng, nm = (int(info[k]) for k in range(5))
    canon, w = np.zeros(NN, np.int64), np.zeros(NN)
    nr, nc, nd = np.zeros(max(nnb, 1), np.int32), np.zeros(max(nnb, 1), np.int32), np.zeros(max(shared, 1), np.int32)
    go, gn = np.zeros(ng + 1, np.int32), np.zeros(max(nm, 1), np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    exa_partition_query_periodic(n, rank, nranks, order, info, vp(canon), vp(w), vp(nr), vp(nc), vp(nd), vp(go), vp(gn))
    nbrs, off = [], 0
    for i in range(nnb):
        nbrs.append((int(nr[i]), nd[off:off + nc[i]].copy()))
        off += nc[i]
    return dict(NN=NN, canon=canon, weight=w, nbrs=nbrs, groups=[gn[go[g]:go[g + 1]].copy() for g in range(ng)],
                group_sizes={2: int(info[5]), 4: int(info[6]), 8: int(info[7])})


# ---- macroscopic tangent of a periodic cell ----------------------------------------------------------------------------------
VOIGT_PAIRS = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))   # the driver's stress order 11, 22, 33, 23, 13, 12


def macro_tangent_voigt(dsig_dL, dt):
    """The 6 x 6 stiffness per strain increment of a (3, 3, 3, 3) tangent d sigma_kl / d L_mn: row I = stress component VOIGT_PAIRS[I], column J = the
    symmetric unit strain of VOIGT_PAIRS[J] (a unit ENGINEERING shear for the off-diagonal pairs: L_mn = L_nm = 1/2), divided by the dt factor
    the operator carries."""
    import numpy as np
    t = np.asarray(dsig_dL, dtype=np.float64).reshape(3, 3, 3, 3)
    c = np.zeros((6, 6))
    for i, (k, l) in enumerate(VOIGT_PAIRS):
        for j, (m, n) in enumerate(VOIGT_PAIRS):
            c[i, j] = 0.5 * (t[k, l, m, n] + t[k, l, n, m]) / dt
    return c


def condense_macro_tangent(dsig_dL, free):
    """Host code: the condensed tangent C_pp - C_pf C_ff^-1 C_fp of the prescribed entries of a mixed run with the (3, 3) free mask, as a
    (3, 3, 3, 3) array with zeros in the free rows and columns."""
    import numpy as np
    c = np.ascontiguousarray(np.asarray(dsig_dL, dtype=np.float64).reshape(81))
    f = (C.c_int * 9)(*[int(bool(v)) for v in np.asarray(free).reshape(9)])
    out = np.zeros(81)
    if exa_macro_tangent_condense(c.ctypes.data_as(_dp), f, out.ctypes.data_as(_dp)) != 0:
        raise RuntimeError("condense_macro_tangent: the block of the free entries is singular")
    return out.reshape(3, 3, 3, 3)


def options_macro_tangent(path):
    """macro_tangent keys of the Visualizations table: dict(enabled, fname, rel_tol, max_iter); rel_tol / max_iter None = the Solvers.Krylov values"""
    o = (C.c_int * 2)()
    rel = C.c_double()
    f = C.create_string_buffer(4096)
    err = C.create_string_buffer(512)
    if exa_options_macro_tangent(path.encode(), o, C.byref(rel), f, 4096, err, 512) != 0:
        raise RuntimeError(err.value.decode())
    return dict(enabled=bool(o[0]), fname=f.value.decode(), rel_tol=rel.value if rel.value > 0 else None, max_iter=int(o[1]) if o[1] > 0 else None)


def write_macro_tangent(path, rows, append=False):
    """rows of (step, time, dt, V, dsig_dL (3, 3, 3, 3)) in the layout of the driver's macro_tangent file (17 significant digits)"""
    import numpy as np
    with open(path, "a" if append else "w") as f:
        for step, t, dt, V, c in rows:
            f.write(" ".join([str(int(step))] + ["%.17g" % v for v in (t, dt, V)] + ["%.17g" % v for v in np.asarray(c, dtype=np.float64).reshape(81)]) + "\n")


def read_macro_tangent(path):
    """a macro_tangent file of the driver: list of dict(step, time, dt, V, dsig_dL (3, 3, 3, 3), C_voigt (6, 6)), one per row"""
    import numpy as np
    out = []
    with open(path) as f:
        for ln in f:
            if not ln.strip() or ln.startswith("#"):
                continue
            v = ln.split()
            if len(v) != 85:
                raise ValueError(f"{path}: a row holds step, time, dt, V and 81 values, not {len(v)} entries")
            c = np.array([float(x) for x in v[4:]]).reshape(3, 3, 3, 3)
            dt = float(v[2])
            out.append(dict(step=int(v[0]), time=float(v[1]), dt=dt, V=float(v[3]), dsig_dL=c, C_voigt=macro_tangent_voigt(c, dt)))
    return out


def tangent_scratch_bytes():
    """private (scratch) bytes per lane of the tangent's kernels in the loaded code object: dict(cols1, cols2, cols3, affine, contract9, contract1, combine)"""
    o = (C.c_int * 8)()
    if exa_tangent_scratch_bytes(o) != 0:
        raise RuntimeError("exa_tangent_scratch_bytes: no device")
    return dict(zip(("cols1", "cols2", "cols3", "affine", "contract9", "contract1", "combine"), [int(v) for v in o[:7]]))


def options_solver(path):
    """Solvers.Krylov preconditioner keys of an options file: dict(preconditioner (None = key absent, "jacobi", "multigrid"), mg_levels, mg_smoother_degree)"""
    out = (C.c_int * 3)()
    err = C.create_string_buffer(512)
    if exa_options_query_solver(path.encode(), out, err, 512) != 0:
        raise RuntimeError(err.value.decode())
    return dict(preconditioner={0: None, 1: "jacobi", 2: "multigrid"}[out[0]], mg_levels=out[1], mg_smoother_degree=out[2])


def mg_level_count(N, nranks=1, cap=0):
    """coarse multigrid levels of an N0 x N1 x N2 element grid on nranks block ranks (0: multigrid refused), capped by cap > 0"""
    n = (C.c_int * 3)(*([int(N)] * 3 if isinstance(N, int) else [int(v) for v in N]))
    return exa_mg_level_count(n, int(nranks), int(cap))


def mg_level_count_order(N, nranks=1, cap=0, order=1):
    """... at polynomial order 1 (mg_level_count) or 2: one more level, the element vertices, which needs no evenness (so never 0)"""
    n = (C.c_int * 3)(*([int(N)] * 3 if isinstance(N, int) else [int(v) for v in N]))
    r = exa_mg_level_count_order(n, int(nranks), int(cap), int(order))
    if r < 0:
        raise ValueError("mg_level_count_order: order 1 or 2, positive sizes")
    return r


def options_mg_p2(path):
    """[Solvers.Krylov] mg_p2 of an options file (read next to preconditioner = "multigrid"): True / False"""
    out = (C.c_int * 1)()
    err = C.create_string_buffer(512)
    if exa_options_query_mg_p2(path.encode(), out, err, 512) != 0:
        raise RuntimeError(err.value.decode())
    return bool(out[0])


def options_mg_bbar(path):
    """[Solvers.Krylov] mg_bbar of an options file (read next to preconditioner = "multigrid"): True / False"""
    out = (C.c_int * 1)()
    err = C.create_string_buffer(512)
    if exa_options_query_mg_bbar(path.encode(), out, err, 512) != 0:
        raise RuntimeError(err.value.decode())
    return bool(out[0])


def mg_p2_bbar_scratch_bytes():
    """private (scratch) bytes per lane of the B-bar forms of the kernels behind exa_grad_mg_p2_build and of their per-element pre-pass in the
    loaded code object: dict of nine (all must be 0)"""
    o = (C.c_int * 9)()
    if exa_mg_p2_bbar_scratch_bytes(o) != 0:
        raise RuntimeError("exa_mg_p2_bbar_scratch_bytes: no device")
    names = [f"{k}_{f}{t}_bbar" for k in ("level1", "diag") for f in ("full", "compact") for t in ("", "_trans")] + ["gbar_prepass"]
    return dict(zip(names, [int(v) for v in o]))


def mg_p2_scratch_bytes():
    """private (scratch) bytes per lane of the kernels behind exa_grad_mg_p2_build in the loaded code object: dict of eight (all must be 0)"""
    o = (C.c_int * 8)()
    if exa_mg_p2_scratch_bytes(o) != 0:
        raise RuntimeError("exa_mg_p2_scratch_bytes: no device")
    names = [f"{k}_{f}{t}" for k in ("level1", "diag") for f in ("full", "compact") for t in ("", "_trans")]
    return dict(zip(names, [int(v) for v in o]))


def options_checkpoint(path):
    """[Checkpoint] table of an options file: dict(write, steps, keep, floc, restart_from)."""
    out = (C.c_int * 3)()
    floc, rst = C.create_string_buffer(4096), C.create_string_buffer(4096)
    err = C.create_string_buffer(512)
    if exa_options_query_checkpoint(path.encode(), out, floc, 4096, rst, 4096, err, 512) != 0:
        raise RuntimeError(err.value.decode())
    return dict(write=bool(out[0]), steps=out[1], keep=out[2], floc=floc.value.decode(), restart_from=rst.value.decode())


def partition_nodes(N, rank, nranks, order=1, mesh=None):
    """Global node number of every local node of a rank's partition (generated N^3 mesh, or the mesh file `mesh`): (node_gid, global node count)."""
    import numpy as np
    info = (C.c_int64 * 2)()
    err = C.create_string_buffer(512)

    def call(buf):
        if mesh is None:
            n = (C.c_int * 3)(*([int(N)] * 3 if isinstance(N, int) else [int(v) for v in N]))
            return exa_partition_query_nodes(n, rank, nranks, order, info, buf)
        return exa_mesh_partition_query_nodes(mesh.encode(), rank, nranks, order, info, buf, err, 512)
    if call(None) != 0:
        raise RuntimeError(err.value.decode())
    gid = np.zeros(info[0], np.int64)
    if call(gid.ctypes.data_as(C.c_void_p)) != 0:
        raise RuntimeError(err.value.decode())
    return gid, int(info[1])


CHECKPOINT_INFO_KEYS = ("version", "elements", "nodes", "qpts_per_elem", "geometry", "order", "model", "nprops", "nstatev", "steps_done", "bc_index",
                        "nranks", "flags", "nsections", "model_calls", "newton_cap", "newton_cap2", "writer")


def checkpoint_info(path):
    """Header and section table of a checkpoint file through the library (no GPU needed): dict of the header fields (CHECKPOINT_INFO_KEYS, time,
    dt_class, last_dt, props_hash, grain_hash, conn_hash, cycle0_saved, texture0_written) and "sections": {name: (offset, nbytes, checksum)}."""
    out, outd, hs = (C.c_int64 * 20)(), (C.c_double * 3)(), (C.c_uint64 * 3)()
    names, info = C.create_string_buffer(24 * 64), (C.c_uint64 * (3 * 64))()
    err = C.create_string_buffer(1024)
    n = exa_checkpoint_info(path.encode(), out, outd, hs, names, info, 64, err, 1024)
    if n < 0:
        raise RuntimeError(err.value.decode())
    d = {k: int(out[i]) for i, k in enumerate(CHECKPOINT_INFO_KEYS)}
    d.update(time=outd[0], dt_class=outd[1], last_dt=outd[2], props_hash=int(hs[0]), grain_hash=int(hs[1]), conn_hash=int(hs[2]),
             cycle0_saved=bool(out[12] & 1), texture0_written=bool(out[12] & 2))
    d["sections"] = {names.raw[24 * i:24 * i + 24].split(b"\0")[0].decode(): (int(info[3 * i]), int(info[3 * i + 1]), int(info[3 * i + 2])) for i in range(min(n, 64))}
    return d


CHECKPOINT_MAGIC = b"EXACKPT\0"
# (name, struct format, byte offset) of the 256-byte header, little-endian
CHECKPOINT_HEADER = (("version", "<I", 8), ("header_bytes", "<I", 12), ("elements", "<q", 16), ("nodes", "<q", 24), ("qpts_per_elem", "<i", 32), ("geometry", "<i", 36),
                     ("order", "<i", 40), ("model", "<i", 44), ("nprops", "<i", 48), ("nstatev", "<i", 52), ("props_hash", "<Q", 56), ("grain_hash", "<Q", 64),
                     ("conn_hash", "<Q", 72), ("steps_done", "<q", 80), ("time", "<d", 88), ("dt_class", "<d", 96), ("last_dt", "<d", 104), ("bc_index", "<i", 112),
                     ("nranks", "<i", 116), ("flags", "<I", 120), ("nsections", "<i", 124), ("model_calls", "<q", 128), ("newton_cap", "<i", 136), ("newton_cap2", "<i", 140),
                     ("writer", "<I", 144))
CHECKPOINT_ROW_WIDTH = {"avg_stress": 6, "avg_def_grad": 9, "avg_pl_work": 1, "avg_dp_tensor": 6, "pvd_cycles": 2, "auto_dt": 1}


def read_checkpoint(path, copy=True):
    """Pure-numpy reader of a checkpoint file, following the documented format and independent of the library: dict with "header"
    (field -> value), "sections" ({name: (offset, nbytes, checksum)}) and one array per section: x_beg / v_sol (nodes, 3) by global node number,
    stress0 (elements, Q, 6) and matVars0 (elements, Q, nstatev) by global element id, avg_* rows, solver_stats (steps, 4) int32
    (Newton iterations, Krylov iterations, constitutive launches, converged), pvd_cycles (n, 2), lattice_strains / lattice_volumes / auto_dt (flat),
    x_beg_copies / v_sol_copies (n, 5) int64 (rank + 2^32 * rank count, global node, bit patterns of the rank's x, y, z).
    Refuses a wrong magic or version, a truncated file and a section whose checksum does not match, naming it.  The file is memory-mapped;
    copy=False returns read-only views of the mapping instead of arrays (a 128^3 checkpoint is 4.7 GB)."""
    import struct
    import numpy as np
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        b = f.read(256)                      # header, then the table; the sections are mapped, not read into a second buffer
        n_ = struct.unpack_from("<i", b, 124)[0] if len(b) == 256 and b[:8] == CHECKPOINT_MAGIC else 0
        b += f.read(48 * max(0, min(n_, 4096)))
    if len(b) < 8 or b[:8] != CHECKPOINT_MAGIC:
        raise ValueError(f"checkpoint: wrong magic ({path} is not a checkpoint file of this library)")
    if len(b) < 256:
        raise ValueError(f"checkpoint: truncated file (the header needs 256 bytes, the file has {size})")
    h = {k: struct.unpack_from(f, b, o)[0] for k, f, o in CHECKPOINT_HEADER}
    if h["version"] != 1 or h["header_bytes"] != 256:
        raise ValueError(f"checkpoint: unsupported format version {h['version']} (this reader reads version 1)")
    with np.errstate(over="ignore"):
        if int(np.frombuffer(b, "<u8", 31, 0).sum(dtype=np.uint64)) != struct.unpack_from("<Q", b, 248)[0]:
            raise ValueError("checkpoint: checksum mismatch in the header")
    n = h["nsections"]
    if len(b) < 256 + 48 * n:
        raise ValueError(f"checkpoint: truncated file (the section table ends at byte {256 + 48 * n}, the file has {size})")
    data = np.memmap(path, dtype=np.uint8, mode="r")
    out = {"header": h, "sections": {}}
    for i in range(n):
        e = 256 + 48 * i
        name = b[e:e + 24].split(b"\0")[0].decode()
        off, nb, cs = struct.unpack_from("<QQQ", b, e + 24)
        if nb and off + nb > size:         # (an empty section holds no bytes wherever its offset points)
            raise ValueError(f"checkpoint: truncated file (section '{name}' ends at byte {off + nb}, the file has {size})")
        words = data[off:off + nb].view("<u8") if nb else np.zeros(0, "<u8")
        with np.errstate(over="ignore"):
            if int(words.sum(dtype=np.uint64)) != cs:
                raise ValueError(f"checkpoint: checksum mismatch in section '{name}'")
        out["sections"][name] = (off, nb, cs)
        E, Q, NN = h["elements"], h["qpts_per_elem"], h["nodes"]
        if name in ("x_beg", "v_sol"):
            a = words.view(np.float64).reshape(NN, 3)
        elif name == "stress0":
            a = words.view(np.float64).reshape(E, Q, 6)
        elif name == "matVars0":
            a = words.view(np.float64).reshape(E, Q, h["nstatev"])
        elif name == "solver_stats":
            a = words.view(np.int32)[:4 * h["steps_done"]].reshape(-1, 4)
        elif name.endswith("_copies"):          # { rank + 2^32 * rank count of the writer, global node, bit patterns of x, y, z } per entry
            a = words.view(np.int64).reshape(-1, 5)
        elif name in CHECKPOINT_ROW_WIDTH:
            a = words.view(np.float64).reshape(-1, CHECKPOINT_ROW_WIDTH[name])
        else:
            a = words.view(np.float64)
        out[name] = np.array(a) if copy else a
    return out


def options_vis(path):
    """Visualizations table of an options file: dict(paraview, steps, light_up, floc)."""
    pv, st, lu = C.c_int(), C.c_int(), C.c_int()
    floc = C.create_string_buffer(4096)
    err = C.create_string_buffer(512)
    if exa_options_query_vis(path.encode(), C.byref(pv), C.byref(st), C.byref(lu), floc, 4096, err, 512) != 0:
        raise RuntimeError(err.value.decode())
    return dict(paraview=bool(pv.value), steps=st.value, light_up=bool(lu.value), floc=floc.value.decode())


def cubic_fiber_axes(h, k, l):
    """distinct unit axes (n, 3) of the cubic plane family {hkl}, a direction and its negative counted once (exa_cubic_fiber_axes)"""
    import numpy as np
    out = np.zeros((24, 3))
    n = exa_cubic_fiber_axes(int(h), int(k), int(l), out.ctypes.data_as(C.POINTER(C.c_double)), 24)
    if n < 0:
        raise ValueError("(0, 0, 0) is not a plane family")
    return out[:n].copy()


def options_grains(path):
    """per-grain averages keys of the Visualizations table: dict(enabled, fname)"""
    en = C.c_int()
    f = C.create_string_buffer(4096)
    err = C.create_string_buffer(512)
    if exa_options_query_grains(path.encode(), C.byref(en), f, 4096, err, 512) != 0:
        raise RuntimeError(err.value.decode())
    return dict(enabled=bool(en.value), fname=f.value.decode())


def options_lightup(path):
    """light-up analysis keys of the Visualizations table: dict(enabled, hkl (list of triples), s_dir, tol_deg, strain_fname, volume_fname)"""
    en, nh = C.c_int(), C.c_int()
    hkl = (C.c_int * 48)()
    sd = (C.c_double * 3)()
    tol = C.c_double()
    f1, f2 = C.create_string_buffer(4096), C.create_string_buffer(4096)
    err = C.create_string_buffer(512)
    if exa_options_query_lightup(path.encode(), C.byref(en), C.byref(nh), hkl, sd, C.byref(tol), f1, f2, 4096, err, 512) != 0:
        raise RuntimeError(err.value.decode())
    return dict(enabled=bool(en.value), hkl=[tuple(hkl[3 * j:3 * j + 3]) for j in range(nh.value)], s_dir=tuple(sd), tol_deg=tol.value,
                strain_fname=f1.value.decode(), volume_fname=f2.value.decode())
exa_mesh_partition_query_order = _sig("exa_mesh_partition_query_order", C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int)
exa_mesh_partition_query = _sig("exa_mesh_partition_query", C.c_int, C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int)
exa_partition_query_boundary_first = _sig("exa_partition_query_boundary_first", C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p)
exa_partition_query = _sig("exa_partition_query", C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)


class Driver:
    """SystemDriver of the reference (src/system_driver.hpp:101-143) running on the GPU behind the C ABI."""

    def __init__(self, handle, errbuf):
        if not handle:
            raise RuntimeError("driver creation failed: " + errbuf.value.decode())
        self.h = handle
        self._err = C.create_string_buffer(512)

    @classmethod
    def from_toml(cls, path, out_dir=".", rank=0, nranks=1, uid=None, jacobi=False, write_files=True, restart=None):
        """restart: a checkpoint file to resume from (overrides Checkpoint.restart_from of the options file); None: what the options file says."""
        err = C.create_string_buffer(1024)
        h = exa_driver_create_restart(path.encode(), out_dir.encode(), rank, nranks, uid, int(jacobi), int(write_files),
                                      None if restart is None else str(restart).encode(), err, 1024)
        return cls(h, err)

    @classmethod
    def synthetic(cls, N, props, quats, dts, bcc=False, slip=0, temp_k=298.0, assembly=0, nrls=False, jacobi=False,
                  newton=(25, 5e-5, 5e-10), krylov=(1000, 1e-7, 1e-27), vz=1.0e-3, rank=0, nranks=1, uid=None, order=1, bbar=False, reversals=()):
        import numpy as np
        props = np.ascontiguousarray(props, dtype=np.float64)
        quats = np.ascontiguousarray(quats, dtype=np.float64)
        dts = np.ascontiguousarray(dts, dtype=np.float64)
        dp = C.POINTER(C.c_double)
        cfg = ExaSynthConfig(N, int(bcc), slip, len(props), props.ctypes.data_as(dp), temp_k, quats.ctypes.data_as(dp), assembly, int(nrls),
                             int(jacobi), newton[0], newton[1], newton[2], krylov[0], krylov[1], krylov[2], len(dts), dts.ctypes.data_as(dp), vz, order, int(bbar),
                             len(reversals), (C.c_int * max(len(reversals), 1))(*[int(r) for r in reversals]))
        err = C.create_string_buffer(512)
        h = exa_driver_create_synthetic(C.byref(cfg), rank, nranks, uid, err, 512)
        return cls(h, err)

    def _chk(self, rc):
        if rc < 0:
            raise RuntimeError(self._err.value.decode())
        return rc

    def step(self, ti, commit=True):
        rc = (exa_driver_step if commit else exa_driver_step_nocommit)(self.h, ti, self._err, 512)
        if rc < 0:
            raise RuntimeError(self._err.value.decode())
        return rc == 1

    def save_checkpoint(self, path):
        """Writes a checkpoint of the current begin-of-step state; every rank of the group calls it."""
        self._chk(exa_driver_save_checkpoint(self.h, str(path).encode(), self._err, 512))

    def load_checkpoint(self, path):
        """Resumes from a checkpoint: legal only on a freshly created driver before its first step; run() continues at the step after the stored one."""
        self._chk(exa_driver_load_checkpoint(self.h, str(path).encode(), self._err, 512))

    def commit_step(self):
        self._chk(exa_driver_commit_step(self.h, self._err, 512))

    def run(self):
        rc = exa_driver_run(self.h, self._err, 512)
        if rc == -1000000:
            raise RuntimeError(self._err.value.decode())
        return rc

    def avgs(self, which, width, maxrows=4096):
        import numpy as np
        out = np.zeros((maxrows, width))
        rows = exa_driver_get_avgs(self.h, which, out.ctypes.data_as(C.POINTER(C.c_double)), maxrows)
        return out[:rows].copy()

    def stats(self, maxrows=4096):
        import numpy as np
        a = [np.zeros(maxrows, np.int32) for _ in range(3)]
        ip = C.POINTER(C.c_int)
        rows = exa_driver_get_stats(self.h, a[0].ctypes.data_as(ip), a[1].ctypes.data_as(ip), a[2].ctypes.data_as(ip), maxrows)
        return [x[:rows].copy() for x in a]

    def timers(self):
        import numpy as np
        t = np.zeros(5)
        exa_driver_get_timers(self.h, t.ctypes.data_as(C.POINTER(C.c_double)))
        return dict(model_ms=t[0], krylov_ms=t[1], solve_ms=t[2], qpt_updates=int(t[3]), krylov_iters=int(t[4]))

    def diagnostics(self):
        import numpy as np
        o = np.zeros(4, np.int64)
        exa_driver_get_diagnostics(self.h, o.ctypes.data_as(C.POINTER(C.c_int64)))
        r = np.zeros(2)
        exa_driver_get_pcg_reduction(self.h, r.ctypes.data_as(C.POINTER(C.c_double)))
        n = np.zeros(2, np.int64)
        exa_driver_get_record_launches(self.h, n.ctypes.data_as(C.POINTER(C.c_int64)))
        return dict(record_policy_launches=int(n[0]), record_generic_launches=int(n[1]), model_failed_points=int(o[0]), pcg_not_converged=int(o[1]), pcg_indefinite_iters=int(o[2]), pcg_last_flag=int(o[3]),
                    pcg_last_reduction=float(r[0]), pcg_worst_capped_reduction=float(r[1]),
                    slip_rate_launches=int(exa_driver_get_rate_launches(self.h)), element_field_launches=int(exa_driver_get_field_launches(self.h)))

    def bench_prepare(self, dts, perturb=1.0, advance=True):
        """Kinematic drive to the state the timed passes start from; advance=False keeps the virgin state (elastic first step, dt = dts[0])."""
        import numpy as np
        dts = np.ascontiguousarray(dts, dtype=np.float64)
        self._chk(exa_driver_bench_prepare(self.h, len(dts) if advance else 0, dts.ctypes.data_as(C.POINTER(C.c_double)), perturb, self._err, 512))

    def nfev_hist(self, which=1):
        """Histogram (64 bins) of the local-solver evaluation counts of the last constitutive launch (which = 1: end-of-step state) or,
        after a completed step, of the launch that step converged with (which = 0: begin-of-step state)."""
        import numpy as np
        h = np.zeros(64, dtype=np.int32)
        self._chk(exa_driver_nfev_hist_of(self.h, which, h.ctypes.data_as(C.POINTER(C.c_int)), self._err, 512))
        return h

    def comm_info(self):
        """(rank count the transport reports - ncclCommCount for RCCL -, transport name)"""
        o = (C.c_int * 2)()
        assert exa_driver_comm_info(self.h, o) == 0
        return int(o[0]), ("none", "rccl", "ipc", "loopback")[o[1]]

    def comm_probe(self, what, vec):
        """The transport on its own: what 0 / 1 / 2 = all-reduce (sum / min / max) of vec, 3 = halo sum of an L-vector of the local dofs.  Every rank calls it."""
        import numpy as np
        v = np.array(vec, dtype=np.float64).ravel()
        assert exa_driver_comm_probe(self.h, int(what), v.ctypes.data_as(C.POINTER(C.c_double)), v.size) == 0
        return v

    def comm_details(self):
        out = (C.c_int64 * 8)()
        assert exa_driver_comm_details(self.h, out) == 0
        return {"elements": int(out[0]), "boundary_block_elements": int(out[1]), "neighbours": int(out[2]), "halo_bytes_per_exchange": 8 * int(out[3]),
                "halo_overlap": bool(out[4])}

    def mesh_info(self):
        """Element geometry and order of this rank's mesh and the route its Krylov action takes (ACTION_ROUTES)."""
        out = (C.c_int64 * 8)()
        assert exa_driver_mesh_info(self.h, out) == 0
        return {"geometry": ("hex", "tet")[out[0]], "order": int(out[1]), "nodes_per_elem": int(out[2]), "qpts_per_elem": int(out[3]),
                "elements": int(out[4]), "nodes": int(out[5]), "action_route": ACTION_ROUTES[out[6]]}

    def reset_timers(self):
        exa_driver_reset_timers(self.h)

    def qf_component(self, which, comp):
        """One component of a quadrature function ([element][point]); which: 0/1 begin/end state, 2/3 begin/end stress."""
        import numpy as np
        out = np.zeros(exa_driver_local_qpts(self.h))
        self._chk(exa_driver_get_qf_component(self.h, which, comp, out.ctypes.data_as(C.c_void_p), self._err, 512))
        return out

    def element_fields(self):
        """Per-element fields of the current begin-of-step state on this rank (after a completed step: the converged one), local element order:
        {field name: array (E, ncomp)} for the ELEMENT_FIELDS names, plus "GlobalElementId" (int64) and "attribute" (grain id, int32)."""
        import numpy as np
        E = self._chk(exa_driver_element_fields(self.h, None, None, None, self._err, 512))
        rows = np.zeros((E, EXA_NFIELDS))
        gid = np.zeros(E, np.int64)
        attr = np.zeros(E, np.int32)
        self._chk(exa_driver_element_fields(self.h, rows.ctypes.data_as(C.POINTER(C.c_double)), gid.ctypes.data_as(C.POINTER(C.c_int64)),
                                            attr.ctypes.data_as(C.POINTER(C.c_int32)), self._err, 512))
        out = {k: rows[:, c0:c0 + n].copy() for k, (c0, n) in ELEMENT_FIELDS.items()}
        out["GlobalElementId"] = gid
        out["attribute"] = attr
        return out

    def lattice_strains(self, hkl, s_dir=(0, 0, 1), tol_deg=5.0):
        """Lattice strains of the plane families hkl (list of [h, k, l]) along the sample direction s_dir on the current begin-of-step state
        (after a completed step: the converged one), over all ranks of the group (every rank calls it): {"strain": (H,), "volume_fraction": (H,)};
        strain is NaN for a fibre without elements within tol_deg degrees."""
        import numpy as np
        h = np.ascontiguousarray(np.asarray(hkl, dtype=np.int32).reshape(-1, 3))
        sd = np.ascontiguousarray(np.asarray(s_dir, dtype=np.float64).reshape(3))
        H = h.shape[0]
        strain, vf = np.zeros(H), np.zeros(H)
        self._chk(exa_driver_lattice_strains(self.h, H, h.ctypes.data_as(C.POINTER(C.c_int)), sd.ctypes.data_as(C.POINTER(C.c_double)), float(tol_deg),
                                             strain.ctypes.data_as(C.POINTER(C.c_double)), vf.ctypes.data_as(C.POINTER(C.c_double)), self._err, 512))
        return {"strain": strain, "volume_fraction": vf}

    def grain_averages(self):
        """Per-grain averages of the current begin-of-step state (after a completed step: the converged one), over all ranks of the
        group (every rank calls it): {"grain_id": (n,), "n_elements", "volume", "volume_fraction", "Stress": (n, 6), "VonMisesStress",
        "HydrostaticStress", "ElasticStrainSample": (n, 6), "XtalElasticStrain": (n, 6), "EffPlasticStrain", "DpEff", "Hardness",
        "ShearRate": (n, 12), "LatticeOrientation": (n, 4), "MisorientationMean", "MisorientationMax", "GrainRotation"} (angles in degrees),
        one row per grain with elements, ascending id."""
        import numpy as np
        cap = getattr(self, "_grain_cap", 4096)       # the row count of the last call: one call in the common case
        while True:
            ids = np.zeros(cap, np.int32)
            vals = np.zeros((cap, EXA_GRAIN_NVALS))
            n = self._chk(exa_driver_grain_averages(self.h, ids.ctypes.data_as(C.POINTER(C.c_int32)), vals.ctypes.data_as(C.POINTER(C.c_double)), cap,
                                                    self._err, 512))
            if n <= cap:
                return grain_dict(ids[:n], vals[:n])
            cap = self._grain_cap = n

    def lattice_curvature(self, burgers=1.0):
        """Intragranular misorientation and lattice curvature of the current begin-of-step state (after a completed step: the
        converged one); every rank of the group calls it.  Rows of this rank in local element order: {"RotationVector": (E, 3) radians,
        "GROD": (E,) degrees, "KAM": (E,) degrees, "LatticeCurvature": (E, 9) row-major kappa_ij in radians per length, "NyeNorm": (E,),
        "GNDDensity": (E,) = NyeNorm / burgers, "GlobalElementId", "attribute"} and "summary": over all ranks the volume-weighted means and
        the maxima named by CURVATURE_SUMMARY, plus "volume"."""
        import numpy as np
        E = self._chk(exa_driver_lattice_curvature(self.h, float(burgers), None, None, None, None, self._err, 512))
        rows = np.zeros((E, EXA_NCURV))
        gid = np.zeros(E, np.int64)
        attr = np.zeros(E, np.int32)
        m = np.zeros(7)
        self._chk(exa_driver_lattice_curvature(self.h, float(burgers), rows.ctypes.data_as(C.POINTER(C.c_double)), gid.ctypes.data_as(C.POINTER(C.c_int64)),
                                               attr.ctypes.data_as(C.POINTER(C.c_int32)), m.ctypes.data_as(C.POINTER(C.c_double)), self._err, 512))
        out = {k: (rows[:, c0].copy() if n == 1 else rows[:, c0:c0 + n].copy()) for k, (c0, n) in CURVATURE_COLUMNS.items()}
        out["GlobalElementId"] = gid
        out["attribute"] = attr
        out["summary"] = dict(zip(CURVATURE_SUMMARY, m[:6].tolist()), volume=float(m[6]))
        return out

    def enable_slip_activity(self):
        """Switches the slip-activity accumulators on, before the first step; an options-file driver does with Visualizations.fatigue."""
        self._chk(exa_driver_enable_slip_activity(self.h, self._err, 512))

    def reset_fatigue_window(self):
        """Asks for a new window of SlipMin / SlipMax / NormalStressMax: it starts with the next committed step (before step 1: at once)."""
        self._chk(exa_driver_reset_fatigue_window(self.h, self._err, 512))

    def slip_activity(self, k=0.5, sigma_y=None):
        """Slip-system activity and the Fatemi-Socie parameter FIP = ShearRange (1 + k NormalStressMax / sigma_y) of the committed state;
        every rank of the group calls it.  Rows of this rank in local element order: {"SlipAccumulated", "SlipAbsolute", "SlipMin", "SlipMax",
        "NormalStressMax": (E, 12) per slip system (the last three over the window), "FIP", "FIPSystem", "ShearRange", "NormalStressMaxFIP" (of the
        FIP system), "AccumulatedSlip", "NetSlipMax": (E,), "GlobalElementId", "attribute"}, "summary": over all ranks the values named by
        FATIGUE_SUMMARY, and "grains": over all ranks {"grain_id", "volume", "FIP_mean", "FIP_max"} per grain with elements."""
        import numpy as np
        if sigma_y is None:
            raise ValueError("slip_activity: sigma_y (the yield stress in the stress unit of the run) is required")
        dp = C.POINTER(C.c_double)
        E = self._chk(exa_driver_slip_activity(self.h, float(k), float(sigma_y), None, None, None, None, None, None, None, 0, None, self._err, 512))
        acc, fip = np.zeros((E, EXA_NSLIPACC)), np.zeros((E, EXA_NFIP))
        gid, attr, m = np.zeros(E, np.int64), np.zeros(E, np.int32), np.zeros(8)
        cap = getattr(self, "_fat_grain_cap", 4096)
        while True:
            ids, vals, n = np.zeros(cap, np.int32), np.zeros((cap, 3)), C.c_int64()
            self._chk(exa_driver_slip_activity(self.h, float(k), float(sigma_y), acc.ctypes.data_as(dp), fip.ctypes.data_as(dp), gid.ctypes.data_as(C.POINTER(C.c_int64)),
                                               attr.ctypes.data_as(C.POINTER(C.c_int32)), m.ctypes.data_as(dp), ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                               vals.ctypes.data_as(dp), cap, C.byref(n), self._err, 512))
            if n.value <= cap:
                break
            cap = self._fat_grain_cap = n.value
        out = {nm: acc[:, 12 * j:12 * j + 12].copy() for j, nm in enumerate(SLIP_ACC_PLANES)}
        for j, nm in enumerate(FIP_COLUMNS):
            out["NormalStressMaxFIP" if nm == "NormalStressMax" else nm] = fip[:, j].copy()
        out["GlobalElementId"] = gid
        out["attribute"] = attr
        out["summary"] = dict(zip(FATIGUE_SUMMARY, m.tolist()))
        for nm in ("FIP_max_element", "window_start_step"):
            out["summary"][nm] = int(out["summary"][nm])
        if n.value > 0:
            out["grains"] = {"grain_id": ids[:n.value].astype(np.int64), "volume": vals[:n.value, 0].copy(), "FIP_mean": vals[:n.value, 1].copy(),
                             "FIP_max": vals[:n.value, 2].copy()}
        return out

    def set_grains(self, grain_ids, quats):
        """Grain map of a synthetic driver before its first step: grain_ids (N^3,) in 1..G by global element index (x fastest), quats (G, 4);
        the elements start from their grain's orientation, which is the grain's reference orientation."""
        import numpy as np
        g = np.ascontiguousarray(np.asarray(grain_ids).reshape(-1), dtype=np.int32)
        q = np.ascontiguousarray(np.asarray(quats, dtype=np.float64).reshape(-1, 4))
        self._chk(exa_driver_set_grains(self.h, g.ctypes.data_as(C.POINTER(C.c_int32)), q.ctypes.data_as(C.POINTER(C.c_double)), q.shape[0], g.size,
                                        self._err, 512))

    def pole_figures(self, hkl=TEXTURE_HKL, ipf_dirs=TEXTURE_IPF_DIRS, res_deg=5.0):
        """Texture of the current begin-of-step state (after a completed step: the converged one), over all ranks of the group
        (every rank calls it), in multiples of random distribution: {"pf": (H, n_alpha, n_beta) pole figures of the families hkl,
        "ipf": (D, n_alpha, n_beta) inverse pole figures of the sample directions ipf_dirs, "alpha_edges", "beta_edges" (degrees),
        "solid_angle": (n_alpha,) of one bin of each ring}."""
        import numpy as np
        h = np.ascontiguousarray(np.asarray(hkl, dtype=np.int32).reshape(-1, 3))
        d = np.ascontiguousarray(np.asarray(ipf_dirs, dtype=np.float64).reshape(-1, 3))
        na, nb = texture_grid(res_deg)
        H, D = h.shape[0], d.shape[0]
        mrd = np.zeros((H + D, na, nb))
        self._chk(exa_driver_pole_figures(self.h, H, h.ctypes.data_as(C.POINTER(C.c_int)), D, d.ctypes.data_as(C.POINTER(C.c_double)), float(res_deg),
                                          mrd.ctypes.data_as(C.POINTER(C.c_double)), self._err, 512))
        ae, be, sa = texture_cells(res_deg)
        return {"pf": mrd[:H].copy(), "ipf": mrd[H:].copy(), "alpha_edges": ae, "beta_edges": be, "solid_angle": sa}

    def write_fields(self, directory, cycle, t):
        """ParaView save of the per-element fields as cycle `cycle` at time t under directory (every rank of a group calls it)."""
        self._chk(exa_driver_write_fields(self.h, str(directory).encode(), cycle, t, self._err, 512))

    def bench_model(self, steps):
        import numpy as np
        o = np.zeros(3)
        self._chk(exa_driver_bench_model(self.h, steps, o.ctypes.data_as(C.POINTER(C.c_double)), self._err, 512))
        return dict(loop_ms=o[0], kernel_ms=o[1], failed=int(o[2]))

    def bench_adapter_route(self, steps, iters):
        """The calls the MFEM adapters make (AOS exa_model_setup, exa_grad_setup, E-vector exa_grad_apply between L->E and E->L) at this driver's state."""
        import numpy as np
        o = np.zeros(24)
        self._chk(exa_driver_bench_adapter_route(self.h, steps, iters, o.ctypes.data_as(C.POINTER(C.c_double)), self._err, 512))
        return dict(model_ms=o[0], pass_ms=o[1], geometry_ms=o[2], grad_setup_ms=o[3], grad_apply_ms=o[4], action_ms=o[5], stress_rel_diff=o[6], state_rel_diff=o[7],
                    action_rel_diff=o[8], failed=int(o[9]), driver_route_model_ms=o[10], driver_route_apply_ms=o[11], aos_staging=bool(o[12]), nfev_differing=int(o[13]),
                    lvec_model_ms=o[14], lvec_apply_ms=o[15], lvec_stress_rel_diff=o[16], lvec_grad_setup_ms=o[17], lvec_action_rel_diff=o[18], lvec_residual_ms=o[19],
                    lvec_records_model_ms=o[20], lvec_records_stress_rel_diff=o[21], lvec_records_action_rel_diff=o[22])

    def bench_pcg(self, iters):
        import numpy as np
        o = np.zeros(3)
        self._chk(exa_driver_bench_pcg(self.h, iters, o.ctypes.data_as(C.POINTER(C.c_double)), self._err, 512))
        return dict(pcg_ms=o[0], iters=int(o[1]), apply_ms=o[2])

    # ---- preconditioner (exa_driver_set_preconditioner) and the multigrid test hooks ---------------------------------------
    def set_preconditioner(self, kind, levels=0, degree=2, periodic=False, p2=False, bbar=False):
        """kind: "identity", "jacobi" or "multigrid" (or 0 / 1 / 2); levels: max coarse levels (0 = as many as the mesh allows); degree: Chebyshev degree;
        periodic=True: multigrid may meet set_periodic, before or after this call (opt-in, like Solvers.Krylov.mg_periodic; refused without it);
        p2=True: multigrid on a generated p = 2 mesh (opt-in, like Solvers.Krylov.mg_p2; refused without it);
        bbar=True: multigrid under the B-bar integrator, at p = 1 and - with p2=True - at p = 2 (opt-in, like Solvers.Krylov.mg_bbar; refused
        without it; it permits and does not require: nothing changes on a FULL driver)"""
        k = PRECOND_KINDS[kind] if isinstance(kind, str) else int(kind)
        if periodic:
            exa_driver_set_mg_periodic(self.h, 1)
        if p2:
            exa_driver_set_mg_p2(self.h, 1)
        if bbar:
            exa_driver_set_mg_bbar(self.h, 1)
        self._chk(exa_driver_set_preconditioner(self.h, k, int(levels), int(degree), self._err, 512))

    def set_periodic(self, vel_grad, free=None):
        """Periodic boundary conditions in all three directions under the macroscopic velocity gradient vel_grad (3, 3), before the
        first step; every rank of the group calls it.  Replaces the prescribed faces of a synthetic driver.  free (3, 3) of 0 / 1: mixed loading
         - a free entry (i, d) is an unknown with zero mean traction component i on face pair d and starts from vel_grad[i, d]."""
        import numpy as np
        L = np.ascontiguousarray(np.asarray(vel_grad, dtype=np.float64).reshape(9))
        if free is None:
            self._chk(exa_driver_set_periodic(self.h, L.ctypes.data_as(_dp), self._err, 512))
            return
        f = np.asarray(free)
        if f.shape != (3, 3):
            raise ValueError("free must be a 3 x 3 mask")
        fm = (C.c_int * 9)(*[int(bool(x)) for x in f.ravel()])
        self._chk(exa_driver_set_periodic_mixed(self.h, L.ctypes.data_as(_dp), fm, self._err, 512))

    def macro_info(self):
        """Mixed loading: dict(free (3, 3) bool, vel_grad (3, 3) the gradient H A^-1 the last solved step realised, period (3, 3) A
        with column d the period vector a_d at the start of that step, resultants (3, 3) F_id of the last converged residual)"""
        import numpy as np
        f = (C.c_int * 9)()
        L, A, F = np.zeros(9), np.zeros(9), np.zeros(9)
        if exa_driver_macro_info(self.h, f, L.ctypes.data_as(_dp), A.ctypes.data_as(_dp), F.ctypes.data_as(_dp)) < 0:
            raise RuntimeError("exa_driver_macro_info failed")
        return dict(free=np.array(list(f), dtype=bool).reshape(3, 3), vel_grad=L.reshape(3, 3), period=A.reshape(3, 3), resultants=F.reshape(3, 3))

    def macro_tangent(self, rel_tol=None, max_iter=None, batched=None):
        """Homogenised tangent of the last solved step of a periodic cell; every rank calls it.  rel_tol / max_iter None: the Krylov
        options; batched None: the automatic route, False: column by column, True: the nine columns in lockstep through the multi-column action.
        dict(dsig_dL (3, 3, 3, 3) = d sigma_kl / d L_mn, C_voigt (6, 6) per strain increment in the order 11, 22, 33, 23, 13, 12 with engineering
        shears, V, dt, iters (9,), flags (9,), reduction (9,) the solver's own, b_norm (9,), true_residual (9,) |b - K_uu w| recomputed by one more
        action, true_rel (9,) their ratio, w_over_a (9,), batched, nch; on a mixed run also free (3, 3) and condensed (3, 3, 3, 3))"""
        import numpy as np
        c, o2, info = np.zeros(81), np.zeros(2), np.zeros((9, 6))
        route = (C.c_int * 2)()
        self._chk(exa_driver_macro_tangent(self.h, 0.0 if rel_tol is None else float(rel_tol), 0 if max_iter is None else int(max_iter),
                                           -1 if batched is None else int(bool(batched)), c.ctypes.data_as(_dp), o2.ctypes.data_as(_dp), info.ctypes.data_as(_dp), route,
                                           self._err, 512))
        c = c.reshape(3, 3, 3, 3)
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(info[:, 3] > 0, info[:, 4] / info[:, 3], 0.0)
        out = dict(dsig_dL=c, C_voigt=macro_tangent_voigt(c, o2[1]), V=float(o2[0]), dt=float(o2[1]), iters=info[:, 0].astype(int), flags=info[:, 1].astype(int),
                   reduction=info[:, 2].copy(), b_norm=info[:, 3].copy(), true_residual=info[:, 4].copy(), true_rel=rel, w_over_a=info[:, 5].copy(),
                   batched=bool(route[0]), nch=int(route[1]))
        mi = self.macro_info()
        if mi["free"].any():
            out["free"] = mi["free"]
            out["condensed"] = condense_macro_tangent(c, mi["free"])
        return out

    def grad_apply_columns(self, x, assembled=False, batched=False, gated=None, y0=None, nch=0):
        """Probe of the operator behind the tangent: x (ncols, local dofs) with dof = node + local nodes * component -> K x, same shape.  assembled:
        the operator K_uu of the tangent's solves instead of the raw element action.  batched: the multi-column action instead of one column at a
        time.  gated (ncols,) bool: those columns are left out and keep y0.  nch: columns per pass of the batched route from now on (0: unchanged)."""
        import numpy as np
        x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
        if x.shape[1] != exa_driver_local_dofs(self.h) or not 1 <= x.shape[0] <= 16:
            raise RuntimeError("grad_apply_columns: x holds 1 to 16 columns of %d local dofs" % exa_driver_local_dofs(self.h))
        y = np.zeros_like(x) if y0 is None else np.ascontiguousarray(y0, dtype=np.float64).copy()
        if y.shape != x.shape:
            raise ValueError("grad_apply_columns: y0 must have the shape of x")
        g = None if gated is None else (C.c_int * x.shape[0])(*[int(bool(v)) for v in gated])
        self._chk(exa_driver_grad_apply_columns(self.h, x.shape[0], x.ctypes.data_as(_dp), y.ctypes.data_as(_dp), (1 if assembled else 0) | (2 if batched else 0), g, int(nch),
                                                self._err, 512))
        return y

    def pcg_solve(self, b, rel_tol, abs_tol, max_iter, check_every=0, graph=None, columns=False):
        """Probe of the linear solver: K_uu x_m = b_m from x = 0 for b (nrhs, local dofs), K_uu the operator of grad_apply_columns(assembled=True), in a
        PCG solver of the probe's own (the run's settings with these tolerances and this cap); every rank calls it.  check_every 0: the run's chunk
        length; graph None: replay as the run decides, False / True: never / at any size.  columns False: the single-system solve for each column in
        turn, by one solver object into one device buffer; True: all columns in lockstep (columns per pass: set_tangent_route).
        dict(x (nrhs, local dofs), iters, flags (1 converged, 2 max_iter, -1 breakdown), reduction the solver's own, indefinite, r0z0, rz the last (r, z))"""
        import numpy as np
        b = np.ascontiguousarray(np.atleast_2d(b), dtype=np.float64)
        if b.shape[1] != exa_driver_local_dofs(self.h) or not 1 <= b.shape[0] <= 16:
            raise RuntimeError("pcg_solve: b holds 1 to 16 columns of %d local dofs" % exa_driver_local_dofs(self.h))
        n = b.shape[0]
        x, red, sc = np.zeros_like(b), np.zeros(n), np.zeros((n, 2))
        it, fl, ind = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        ip = C.POINTER(C.c_int)
        self._chk(exa_driver_pcg_solve(self.h, n, b.ctypes.data_as(_dp), float(rel_tol), float(abs_tol), int(max_iter), int(check_every), -1 if graph is None else int(bool(graph)),
                                       int(bool(columns)), x.ctypes.data_as(_dp), it.ctypes.data_as(ip), fl.ctypes.data_as(ip), red.ctypes.data_as(_dp), ind.ctypes.data_as(ip),
                                       sc.ctypes.data_as(_dp), self._err, 512))
        return dict(x=x, iters=it.astype(int), flags=fl.astype(int), reduction=red, indefinite=ind.astype(int), r0z0=sc[:, 0].copy(), rz=sc[:, 1].copy())

    def set_krylov(self, solver, kdim=50):
        """The run's linear solver: "pcg", or "gmres" with the Krylov dimension kdim (1 ... 100) of a restart cycle.  Before the first
        step or between steps; every rank calls it.  Tolerances and cap stay; the run's diagnostics() and timers() go on counting (the restarts and
        reorth_passes of krylov_info() are the new GMRES object's)."""
        self._chk(exa_driver_set_krylov(self.h, str(solver).encode(), int(kdim), self._err, 512))

    def krylov_info(self):
        """dict(solver "pcg" / "gmres", kdim (0 for PCG), multidot_chunk: basis vectors per pass of the multi-dot kernel, restarts and reorth_passes over
        all solves of the run's solver, basis_bytes: device memory of its basis, 0 before the first GMRES solve)"""
        i3, o3 = (C.c_int * 3)(), (C.c_int64 * 3)()
        assert exa_driver_krylov_info(self.h, i3, o3) == 0
        return dict(solver="gmres" if i3[0] else "pcg", kdim=int(i3[1]), multidot_chunk=int(i3[2]), restarts=int(o3[0]), reorth_passes=int(o3[1]), basis_bytes=int(o3[2]))

    def gmres_solve(self, b, rel_tol, abs_tol, max_iter, kdim, check_every=0, ortho=None):
        """Probe of GMRES(kdim), as pcg_solve: K_uu x_m = b_m from x = 0 for b (nrhs, local dofs) in turn, in a solver of the probe's own with the run's
        preconditioner; every rank calls it.  ortho None: as EXA_GMRES_ORTHO says; "ifneeded", "always", "never", "mgs".
        dict(x, iters (Arnoldi steps), flags (1 converged, 2 max_iter, -1 breakdown), reduction = resid / beta0, beta0 = |M^-1 b|, resid the last
        residual norm, restarts, reorth_passes)"""
        import numpy as np
        b = np.ascontiguousarray(np.atleast_2d(b), dtype=np.float64)
        if b.shape[1] != exa_driver_local_dofs(self.h) or not 1 <= b.shape[0] <= 16:
            raise RuntimeError("gmres_solve: b holds 1 to 16 columns of %d local dofs" % exa_driver_local_dofs(self.h))
        n = b.shape[0]
        x, red, sc = np.zeros_like(b), np.zeros(n), np.zeros((n, 4))
        it, fl = np.zeros(n, np.int32), np.zeros(n, np.int32)
        ip = C.POINTER(C.c_int)
        self._chk(exa_driver_gmres_solve(self.h, n, b.ctypes.data_as(_dp), float(rel_tol), float(abs_tol), int(max_iter), int(kdim), int(check_every),
                                         -1 if ortho is None else GMRES_ORTHO[ortho], x.ctypes.data_as(_dp), it.ctypes.data_as(ip), fl.ctypes.data_as(ip), red.ctypes.data_as(_dp),
                                         sc.ctypes.data_as(_dp), self._err, 512))
        return dict(x=x, iters=it.astype(int), flags=fl.astype(int), reduction=red, beta0=sc[:, 0].copy(), resid=sc[:, 1].copy(), restarts=sc[:, 2].astype(int),
                    reorth_passes=sc[:, 3].astype(int))

    def set_tangent_route(self, nch=0, auto_batched=True):
        assert exa_driver_set_tangent_route(self.h, int(nch), int(bool(auto_batched))) == 0

    def periodic_info(self):
        """dict(enabled, groups {2: n, 4: n, 8: n} local periodic groups by image count, shared: canonical ids exchanged with other ranks,
        neighbours, vel_grad (3, 3) in force)"""
        import numpy as np
        o = (C.c_int64 * 8)()
        L = np.zeros(9)
        assert exa_driver_periodic_info(self.h, o, L.ctypes.data_as(_dp)) == 0
        return dict(enabled=bool(o[0]), groups={2: int(o[1]), 4: int(o[2]), 8: int(o[3])}, shared=int(o[4]), neighbours=int(o[5]), vel_grad=L.reshape(3, 3))

    def nodal_field(self, name):
        """"velocity", "coords" (current; after a completed step: its end) or "coords_ref" of this rank's nodes: (NN_local, 3); row g belongs to the
        node partition_nodes() numbers node_gid[g]"""
        import numpy as np
        which = NODAL_FIELDS[name]
        nn = self._chk(exa_driver_get_nodal(self.h, which, None, self._err, 512))
        out = np.zeros((nn, 3))
        self._chk(exa_driver_get_nodal(self.h, which, out.ctypes.data_as(_dp), self._err, 512))
        return out

    def newton_info(self):
        """dict(norm: residual norm the last Newton solve of the last step ended with, bound: max(rel_tol |r0|, abs_tol) it had to reach)"""
        o = (C.c_double * 2)()
        exa_driver_newton_info(self.h, o)
        return dict(norm=float(o[0]), bound=float(o[1]))

    def mg_info(self):
        """dict(levels, setup_ms, vcycle_ms, degree, boxes (L+1, 3) local elements per direction, lmax (L+1,), periodic, control_dofs: free
        control entries of mixed loading the preconditioner scales by their diagonal, order (L+1,), level1_build "records" / "probe" / None,
        bbar: the fine operator is the B-bar one)"""
        import numpy as np
        out = np.zeros(6 + 4 * 32)
        if exa_driver_mg_info(self.h, out.ctypes.data_as(_dp)) != 0:
            raise RuntimeError("exa_driver_mg_info failed (no multigrid preconditioner)")
        L = int(out[0])
        per = out[4:4 + 4 * (L + 1)].reshape(L + 1, 4)
        oi = (C.c_int * 40)()
        if exa_driver_mg_info_order(self.h, oi) != 0:
            raise RuntimeError("exa_driver_mg_info_order failed (no multigrid preconditioner)")
        return dict(levels=L, setup_ms=float(out[1]), vcycle_ms=float(out[2]), degree=int(out[3]), boxes=per[:, :3].astype(int), lmax=per[:, 3].copy(),
                    periodic=bool(out[4 + 4 * (L + 1)]), control_dofs=int(out[5 + 4 * (L + 1)]), order=[int(oi[2 + l]) for l in range(L + 1)],
                    level1_build={1: "records", 0: "probe"}.get(int(oi[1])), bbar=exa_driver_mg_bbar(self.h) == 1)

    def set_mg_p2_build(self, from_records=True):
        """p = 2 hierarchy, from the next set-up on: level 1 and the fine diagonal from the point records where they can serve (default), or
        always by probing (False: what the records build is compared against)"""
        exa_driver_set_mg_p2_build(self.h, 1 if from_records else 0)

    def mg_setup(self):
        """gradient set-up of the current state + hierarchy build (the hooks then act on the operator the driver holds now)"""
        self._chk(exa_driver_mg_setup(self.h, self._err, 512))

    def mg_level_dofs(self, level):
        n = exa_driver_mg_level_dofs(self.h, int(level))
        if n < 0:
            raise RuntimeError(f"no multigrid level {level}")
        return int(n)

    def _mg_vec(self, level, x):
        import numpy as np
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.size != self.mg_level_dofs(level):
            raise ValueError(f"level {level} holds {self.mg_level_dofs(level)} dofs, got {x.size}")
        return x

    def mg_apply(self, level, x):
        """y = A_level x (level 0: the constrained operator the PCG applies)"""
        import numpy as np
        x = self._mg_vec(level, x)
        y = np.empty_like(x)
        if exa_driver_mg_apply(self.h, int(level), x.ctypes.data_as(_dp), y.ctypes.data_as(_dp)) != 0:
            raise RuntimeError("exa_driver_mg_apply failed")
        return y

    def mg_diag(self, level):
        import numpy as np
        y = np.empty(self.mg_level_dofs(level))
        if exa_driver_mg_diag(self.h, int(level), y.ctypes.data_as(_dp)) != 0:
            raise RuntimeError("exa_driver_mg_diag failed")
        return y

    def mg_transfer(self, level, direction, x):
        """direction 0: P x (level + 1 -> level); 1: restriction (level -> level + 1)"""
        import numpy as np
        x = self._mg_vec(level + 1 if direction == 0 else level, x)
        y = np.empty(self.mg_level_dofs(level if direction == 0 else level + 1))
        if exa_driver_mg_transfer(self.h, int(level), int(direction), x.ctypes.data_as(_dp), y.ctypes.data_as(_dp)) != 0:
            raise RuntimeError("exa_driver_mg_transfer failed")
        return y

    def mg_stencil(self, level):
        """stored coarse operator of level >= 1: (243, nodes), row (o * 9 + 3 r + c)"""
        import numpy as np
        out = np.empty(243 * (self.mg_level_dofs(level) // 3))
        if exa_driver_mg_stencil(self.h, int(level), out.ctypes.data_as(_dp)) != 0:
            raise RuntimeError("exa_driver_mg_stencil failed")
        return out.reshape(243, -1)

    def precond_apply(self, r):
        """z = B r, one multigrid V-cycle"""
        import numpy as np
        r = self._mg_vec(0, r)
        z = np.empty_like(r)
        if exa_driver_precond_apply(self.h, r.ctypes.data_as(_dp), z.ctypes.data_as(_dp)) != 0:
            raise RuntimeError("exa_driver_precond_apply failed")
        return z

    def close(self):
        if self.h:
            exa_driver_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
