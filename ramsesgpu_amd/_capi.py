"""ctypes view of include/rgpu.h (the C ABI) -- plain structs and prototypes, no compute here."""
import ctypes as C

RGPU_ABI_VERSION = 5

ID, IP, IU, IV, IW, IA, IB, IC = range(8)
BC_UNDEFINED, BC_DIRICHLET, BC_NEUMANN, BC_PERIODIC, BC_SHEARINGBOX, BC_COPY, BC_Z_STRATIFIED = range(7)
RS_APPROX, RS_HLL, RS_HLLC, RS_HLLD, RS_LLF = range(5)
XDIR, YDIR, ZDIR = 1, 2, 3
# the columns of a monitor (rgpu_state_monitor, rgpu_ensemble_monitor, rgpu_ensemble_run_steps_monitored): RGPU_MON_NQ = 10
MON_NAMES = ("mass", "mx", "my", "mz", "E", "ekin", "emag", "min_rho", "min_eint", "max_absdivb")
MON_NQ = len(MON_NAMES)
# the columns of a row of the plane monitor (rgpu_state_monitor_planes, rgpu_run_steps_monitored_planes): RGPU_MONP_NQ = 16
MONP_NAMES = MON_NAMES + ("bx", "by", "bz", "bxby", "rvxvy", "rho2")
MONP_NQ = len(MONP_NAMES)
# the channels of a map (rgpu_state_maps, rgpu_run_steps_mapped): RGPU_MAP_NQ = 12, columns 0 1 2 3 4 5 6 8 10 11 12 15 of the plane monitor's terms
MAP_NAMES = ("rho", "mx", "my", "mz", "E", "ekin", "emag", "eint", "bx", "by", "bz", "rho2")
MAP_NQ = len(MAP_NAMES)
MAP_MAX = 8
# the channels of a PDF (rgpu_state_pdfs, rgpu_run_steps_pdfs): RGPU_PDF_NQ = 13, columns 0 1 2 3 4 5 6 8 10 11 12 9 of the plane monitor's terms, then v2
PDF_NAMES = ("rho", "mx", "my", "mz", "E", "ekin", "emag", "eint", "bx", "by", "bz", "absdivb", "v2")
PDF_NQ = len(PDF_NAMES)
PDF_MAX = 8
PDF_MAX_WORDS = 16384
# the channels of a spectrum (rgpu_state_spectra, rgpu_run_steps_spectra): RGPU_SPECTRUM_NQ = 13, bit q of a spec's mask is channel q
SPECTRUM_NAMES = ("rho", "mx", "my", "mz", "vx", "vy", "vz", "wx", "wy", "wz", "bx", "by", "bz")
SPECTRUM_NQ = len(SPECTRUM_NAMES)
SPECTRUM_MAX = 4
SPECTRUM_MAX_SHELLS = 4096
SPECTRUM_MAX_WEIGHT = 64
# the vector fields of a Helmholtz spectrum (rgpu_state_helm_spectra, rgpu_run_steps_helm_spectra): RGPU_HELM_NF = 4, the channel
# triples 1-3, 4-6, 7-9, 10-12 of SPECTRUM_NAMES
HELM_NAMES = ("m", "v", "w", "b")
HELM_NF = len(HELM_NAMES)
HELM_MAX = 4
T_NAMES = ["boundaries", "prim", "elec", "trace", "flux", "emf", "update", "shear", "dt", "dissipative", "sweep"]


class RgpuParams(C.Structure):
    """struct rgpu_params (include/rgpu.h) -- field order and types must match exactly."""
    _fields_ = [
        ("abi_version", C.c_int32),
        ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32),
        ("ghostWidth", C.c_int32),
        ("nbVar", C.c_int32),
        ("mhdEnabled", C.c_int32),
        ("bc", C.c_int32 * 6),
        ("xMin", C.c_double), ("xMax", C.c_double), ("yMin", C.c_double), ("yMax", C.c_double),
        ("zMin", C.c_double), ("zMax", C.c_double),
        ("dx", C.c_double), ("dy", C.c_double), ("dz", C.c_double),
        ("cfl", C.c_double),
        ("gamma0", C.c_double), ("cIso", C.c_double), ("smallr", C.c_double), ("smallc", C.c_double),
        ("smalle", C.c_double), ("smallp", C.c_double), ("smallpp", C.c_double), ("gamma6", C.c_double),
        ("Omega0", C.c_double),
        ("slope_type", C.c_double),
        ("niter_riemann", C.c_int32), ("iorder", C.c_int32),
        ("riemannSolver", C.c_int32),
        ("magRiemannSolver", C.c_int32),
        ("implementationVersion", C.c_int32),
        ("unsplitVersion", C.c_int32),
        ("shearingBoxEnabled", C.c_int32),
        ("enableJet", C.c_int32), ("ijet", C.c_int32), ("offsetJet", C.c_int32),
        ("djet", C.c_double), ("ujet", C.c_double), ("pjet", C.c_double), ("cjet", C.c_double),
        ("slab_rank", C.c_int32), ("slab_count", C.c_int32),
        ("nz_global", C.c_int32),
        ("gravityEnabled", C.c_int32),
        ("gravity_x", C.c_double), ("gravity_y", C.c_double), ("gravity_z", C.c_double),
        ("nu", C.c_double), ("eta", C.c_double),
        ("zStratifiedFloor", C.c_int32), ("randomForcingEnabled", C.c_int32), ("randomForcingEdot", C.c_double),
        ("ouForcingEnabled", C.c_int32), ("ouInitRandom", C.c_int32),
        ("ouTimeScaleTurb", C.c_double), ("ouAmplitudeTurb", C.c_double), ("ouKsi", C.c_double),
    ]

    @property
    def three_d(self):
        return self.nz_global != 1

    @property
    def shape(self):
        """(nbVar, ksize, jsize, isize) of a ghost-inclusive state array."""
        gw = self.ghostWidth
        ks = self.nz + 2 * gw if self.three_d else 1
        return (self.nbVar, ks, self.ny + 2 * gw, self.nx + 2 * gw)

    def copy(self):
        q = RgpuParams()
        C.memmove(C.byref(q), C.byref(self), C.sizeof(RgpuParams))
        return q


c_double_p = C.POINTER(C.c_double)


class RgpuMapSpec(C.Structure):
    """rgpu_map_spec: axis 0 = x, 1 = y, 2 = z, the direction summed over; [lo, hi) in interior indices along it"""
    _fields_ = [("axis", C.c_int), ("lo", C.c_int), ("hi", C.c_int)]


class RgpuPdfAxis(C.Structure):
    """rgpu_pdf_axis: the channel; scale 0 linear bins on [lo, hi), 1 octave bins on |x| with 2^sub sub-bins each, lo and hi powers of two"""
    _fields_ = [("channel", C.c_int), ("scale", C.c_int), ("nbins", C.c_int), ("sub", C.c_int), ("lo", C.c_double), ("hi", C.c_double)]


class RgpuPdfSpec(C.Structure):
    """rgpu_pdf_spec: b.nbins == 0: the 1D histogram of a; else the joint table [a.nbins + 3][b.nbins + 3]"""
    _fields_ = [("a", RgpuPdfAxis), ("b", RgpuPdfAxis)]


class RgpuSpectrumSpec(C.Structure):
    """rgpu_spectrum_spec: the bit mask of the channels and the integer weights of the shell rule"""
    _fields_ = [("channels", C.c_uint), ("wx", C.c_int), ("wy", C.c_int), ("wz", C.c_int)]


class RgpuHelmSpec(C.Structure):
    """rgpu_helm_spec: the vector field (an index into HELM_NAMES) and the integer weights, none of them zero"""
    _fields_ = [("field", C.c_int), ("wx", C.c_int), ("wy", C.c_int), ("wz", C.c_int)]


def declare_host_api(lib):
    """prototypes of the rgpuh_* entry points + rgpu_state_elems"""
    lib.rgpu_state_elems.restype = C.c_size_t
    lib.rgpu_state_elems.argtypes = [C.POINTER(RgpuParams)]
    lib.rgpuh_params_from_ini.restype = C.c_int
    lib.rgpuh_params_from_ini.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(RgpuParams), C.c_char_p, C.c_int]
    lib.rgpuh_run_settings.restype = C.c_int
    lib.rgpuh_run_settings.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_int), c_double_p, C.POINTER(C.c_int),
                                       C.c_char_p, C.c_int]
    lib.rgpuh_init_condition.restype = C.c_int
    lib.rgpuh_init_condition.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(RgpuParams), C.c_void_p, C.c_char_p, C.c_int]
    lib.rgpuh_init_forcing.restype = C.c_int
    lib.rgpuh_init_forcing.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(RgpuParams), C.c_void_p, C.c_char_p, C.c_int]
    lib.rgpuh_init_gravity.restype = C.c_int
    lib.rgpuh_init_gravity.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(RgpuParams), C.c_void_p, C.c_char_p, C.c_int]
    return lib


def declare_device_api(lib):
    """prototypes of the rgpu_* entry points (include/rgpu.h)"""
    P = C.POINTER(RgpuParams)
    ctx = C.c_void_p
    lib.rgpu_create.restype = C.c_int
    lib.rgpu_create.argtypes = [P, C.POINTER(ctx)]
    lib.rgpu_create_external.restype = C.c_int
    lib.rgpu_create_external.argtypes = [P, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ctx)]
    lib.rgpu_destroy.restype = None
    lib.rgpu_destroy.argtypes = [ctx]
    lib.rgpu_device_bytes.restype = C.c_size_t
    lib.rgpu_device_bytes.argtypes = [P]
    lib.rgpu_last_error.restype = C.c_char_p
    lib.rgpu_last_error.argtypes = [ctx]
    lib.rgpu_upload.restype = C.c_int
    lib.rgpu_upload.argtypes = [ctx, C.c_void_p, C.c_int]
    lib.rgpu_download.restype = C.c_int
    lib.rgpu_download.argtypes = [ctx, C.c_void_p, C.c_int]
    lib.rgpu_device_state.restype = C.c_void_p
    lib.rgpu_device_state.argtypes = [ctx, C.c_int]
    lib.rgpu_state_checksum.restype = C.c_int
    lib.rgpu_state_checksum.argtypes = [ctx, C.c_int, C.POINTER(C.c_ulonglong)]
    lib.rgpu_history_turbulence.restype = C.c_int
    lib.rgpu_history_turbulence.argtypes = [ctx, C.c_int, c_double_p]
    lib.rgpu_step_ou_forcing.restype = C.c_int
    lib.rgpu_step_ou_forcing.argtypes = [ctx, C.c_int, C.c_double]
    lib.rgpu_ou_forcing_get_state.restype = C.c_int
    lib.rgpu_ou_forcing_get_state.argtypes = [ctx, c_double_p]
    lib.rgpu_ou_forcing_set_state.restype = C.c_int
    lib.rgpu_ou_forcing_set_state.argtypes = [ctx, c_double_p]
    lib.rgpu_ou_forcing_state.restype = C.c_int
    lib.rgpu_ou_forcing_state.argtypes = [ctx, c_double_p, c_double_p]
    lib.rgpu_get_params.restype = C.c_int
    lib.rgpu_get_params.argtypes = [ctx, P]
    lib.rgpu_stream_handle.restype = C.c_void_p
    lib.rgpu_stream_handle.argtypes = [ctx]
    lib.rgpu_inv_dt_device_slot.restype = C.c_void_p
    lib.rgpu_inv_dt_device_slot.argtypes = [ctx]
    lib.rgpu_make_boundaries.restype = C.c_int
    lib.rgpu_make_boundaries.argtypes = [ctx, C.c_int, C.c_int]
    lib.rgpu_make_boundaries_shear.restype = C.c_int
    lib.rgpu_make_boundaries_shear.argtypes = [ctx, C.c_int, C.c_double, C.c_double]
    lib.rgpu_make_all_boundaries.restype = C.c_int
    lib.rgpu_make_all_boundaries.argtypes = [ctx, C.c_int, C.c_double, C.c_double]
    lib.rgpu_compute_inv_dt.restype = C.c_int
    lib.rgpu_compute_inv_dt.argtypes = [ctx, C.c_int, c_double_p]
    lib.rgpu_history_columns.restype = C.c_int
    lib.rgpu_history_columns.argtypes = [ctx, C.c_int, c_double_p]
    lib.rgpu_history_reynolds.restype = C.c_int
    lib.rgpu_history_reynolds.argtypes = [ctx, C.c_int, c_double_p, c_double_p, C.c_double, c_double_p]
    lib.rgpu_set_forcing_field.restype = C.c_int
    lib.rgpu_set_forcing_field.argtypes = [ctx, C.c_void_p]
    lib.rgpu_forcing_sums.restype = C.c_int
    lib.rgpu_forcing_sums.argtypes = [ctx, C.c_int, c_double_p]
    lib.rgpu_add_forcing.restype = C.c_int
    lib.rgpu_add_forcing.argtypes = [ctx, C.c_int, C.c_double]
    lib.rgpu_set_gravity_field.restype = C.c_int
    lib.rgpu_set_gravity_field.argtypes = [ctx, C.c_void_p]
    lib.rgpu_history_mri.restype = C.c_int
    lib.rgpu_history_mri.argtypes = [ctx, C.c_int, c_double_p]
    lib.rgpu_read_cell.restype = C.c_int
    lib.rgpu_read_cell.argtypes = [ctx, C.c_int, C.c_int, C.c_int, C.c_int, c_double_p]
    lib.rgpu_invalidate_dt.restype = C.c_int
    lib.rgpu_invalidate_dt.argtypes = [ctx]
    lib.rgpu_compute_dt.restype = C.c_double
    lib.rgpu_compute_dt.argtypes = [ctx, C.c_int]
    lib.rgpu_inv_dt_fused_active.restype = C.c_int
    lib.rgpu_inv_dt_fused_active.argtypes = [C.c_void_p, C.c_int]
    lib.rgpu_inv_dt_fused_commit.restype = C.c_int
    lib.rgpu_inv_dt_fused_commit.argtypes = [C.c_void_p, C.c_int]
    lib.rgpu_step_core_planes_split.restype = C.c_int
    lib.rgpu_step_core_planes_split.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int]
    lib.rgpu_step_core_planes_pair.restype = C.c_int
    lib.rgpu_step_core_planes_pair.argtypes = [ctx, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.rgpu_step_fill_planes_pair.restype = C.c_int
    lib.rgpu_step_fill_planes_pair.argtypes = [ctx, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int]
    for name in ("rgpu_step_core_planes", "rgpu_step_fill_planes"):
        f = getattr(lib, name)
        f.restype = C.c_int
        f.argtypes = [ctx, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int]
    lib.rgpu_inv_dt_accumulate.restype = C.c_int
    lib.rgpu_inv_dt_accumulate.argtypes = [ctx, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.rgpu_inv_dt_result.restype = C.c_int
    lib.rgpu_inv_dt_result.argtypes = [ctx, c_double_p]
    for name in ("rgpu_godunov_unsplit", "rgpu_step_pre", "rgpu_step_core", "rgpu_step_dissipative", "rgpu_step_post_a", "rgpu_step_post_b"):
        fn = getattr(lib, name)
        fn.restype = C.c_int
        fn.argtypes = [ctx, C.c_int, C.c_double, C.c_double]
    lib.rgpu_one_step_integration.restype = C.c_int
    lib.rgpu_one_step_integration.argtypes = [ctx, C.POINTER(C.c_int), c_double_p, c_double_p]
    lib.rgpu_device_time_step_ready.restype = C.c_int
    lib.rgpu_device_time_step_ready.argtypes = [ctx, C.c_int]
    lib.rgpu_run_steps_log.restype = C.c_int
    lib.rgpu_run_steps_log.argtypes = [ctx, C.c_int, C.c_double, C.POINTER(C.c_int), c_double_p, c_double_p, c_double_p]
    lib.rgpu_run_steps_history.restype = C.c_int
    lib.rgpu_run_steps_history.argtypes = [ctx, C.c_int, C.c_double, C.POINTER(C.c_int), c_double_p, c_double_p, c_double_p, C.c_double, c_double_p,
                                           C.POINTER(C.c_int), C.POINTER(C.c_int), c_double_p, c_double_p, c_double_p]
    lib.rgpu_history_batch_heads.restype = C.c_long
    lib.rgpu_history_batch_heads.argtypes = [ctx]
    lib.rgpu_forcing_batch_steps.restype = C.c_long
    lib.rgpu_forcing_batch_steps.argtypes = [ctx]
    lib.rgpu_run_steps.restype = C.c_int
    lib.rgpu_run_steps.argtypes = [ctx, C.c_int, C.c_double, C.POINTER(C.c_int), c_double_p, c_double_p]
    lib.rgpu_synchronize.restype = C.c_int
    lib.rgpu_synchronize.argtypes = [ctx]
    lib.rgpu_enable_timers.restype = C.c_int
    lib.rgpu_enable_timers.argtypes = [ctx, C.c_int]
    lib.rgpu_get_timers.restype = C.c_int
    lib.rgpu_get_timers.argtypes = [ctx, c_double_p, C.c_int]
    lib.rgpu_reset_timers.restype = C.c_int
    lib.rgpu_reset_timers.argtypes = [ctx]
    lib.rgpu_timer_name.restype = C.c_char_p
    lib.rgpu_timer_name.argtypes = [C.c_int]
    lib.rgpu_dominant_kernel.restype = C.c_int
    lib.rgpu_dominant_kernel.argtypes = [ctx, C.c_char_p, C.c_int, c_double_p, C.POINTER(C.c_long)]
    lib.rgpu_backend_name.restype = C.c_char_p
    lib.rgpu_backend_name.argtypes = []
    lib.rgpu_arithmetic.restype = C.c_char_p
    lib.rgpu_arithmetic.argtypes = []
    lib.rgpu_set_option.restype = C.c_int
    lib.rgpu_set_option.argtypes = [C.c_char_p, C.c_int]
    lib.rgpu_get_option.restype = C.c_int
    lib.rgpu_get_option.argtypes = [C.c_char_p]
    lib.rgpu_clock_check.restype = C.c_int
    lib.rgpu_clock_check.argtypes = [ctx]
    lib.rgpu_state_monitor.restype = C.c_int
    lib.rgpu_state_monitor.argtypes = [ctx, C.c_int, c_double_p]
    if hasattr(lib, "rgpu_state_monitor3d"):   # (absent from an older build of the library: scripts/monitor_bench.py --baseline-lib)
        lib.rgpu_state_monitor3d.restype = C.c_int
        lib.rgpu_state_monitor3d.argtypes = [ctx, C.c_int, c_double_p]
        lib.rgpu_run_steps_monitored.restype = C.c_int
        lib.rgpu_run_steps_monitored.argtypes = [ctx, C.c_int, C.c_double, C.POINTER(C.c_int), c_double_p, c_double_p, c_double_p, C.c_int,
                                                 C.POINTER(C.c_int), C.POINTER(C.c_int), c_double_p, c_double_p]
        lib.rgpu_monitor_batch_samples.restype = C.c_long
        lib.rgpu_monitor_batch_samples.argtypes = [ctx]
    if hasattr(lib, "rgpu_state_monitor_planes"):   # (absent from an older build of the library: scripts/monitor_planes_bench.py --baseline-lib)
        lib.rgpu_state_monitor_planes.restype = C.c_int
        lib.rgpu_state_monitor_planes.argtypes = [ctx, C.c_int, c_double_p]
        lib.rgpu_run_steps_monitored_planes.restype = C.c_int
        lib.rgpu_run_steps_monitored_planes.argtypes = [ctx, C.c_int, C.c_double, C.POINTER(C.c_int), c_double_p, c_double_p, c_double_p, C.c_int,
                                                        C.POINTER(C.c_int), C.POINTER(C.c_int), c_double_p, c_double_p]
        lib.rgpu_monitor_planes_batch_samples.restype = C.c_long
        lib.rgpu_monitor_planes_batch_samples.argtypes = [ctx]
    if hasattr(lib, "rgpu_state_maps"):   # (absent from an older build of the library: scripts/monitor_maps_bench.py --baseline-lib)
        lib.rgpu_map_doubles.restype = C.c_size_t
        lib.rgpu_map_doubles.argtypes = [ctx, C.POINTER(RgpuMapSpec)]
        lib.rgpu_state_maps.restype = C.c_int
        lib.rgpu_state_maps.argtypes = [ctx, C.c_int, C.c_int, C.POINTER(RgpuMapSpec), c_double_p]
        lib.rgpu_run_steps_mapped.restype = C.c_int
        lib.rgpu_run_steps_mapped.argtypes = [ctx, C.c_int, C.c_double, C.POINTER(C.c_int), c_double_p, c_double_p, c_double_p, C.c_int,
                                              C.c_int, C.POINTER(RgpuMapSpec), C.POINTER(C.c_int), C.POINTER(C.c_int), c_double_p, c_double_p]
        lib.rgpu_map_batch_samples.restype = C.c_long
        lib.rgpu_map_batch_samples.argtypes = [ctx]
    if hasattr(lib, "rgpu_state_pdfs"):   # (absent from an older build of the library)
        c_u64_p = C.POINTER(C.c_ulonglong)
        lib.rgpu_pdf_words.restype = C.c_size_t
        lib.rgpu_pdf_words.argtypes = [C.POINTER(RgpuPdfSpec)]
        lib.rgpu_state_pdfs.restype = C.c_int
        lib.rgpu_state_pdfs.argtypes = [ctx, C.c_int, C.c_int, C.POINTER(RgpuPdfSpec), c_u64_p]
        lib.rgpu_run_steps_pdfs.restype = C.c_int
        lib.rgpu_run_steps_pdfs.argtypes = [ctx, C.c_int, C.c_double, C.POINTER(C.c_int), c_double_p, c_double_p, c_double_p, C.c_int,
                                            C.c_int, C.POINTER(RgpuPdfSpec), C.POINTER(C.c_int), C.POINTER(C.c_int), c_double_p, c_u64_p]
        lib.rgpu_pdf_batch_samples.restype = C.c_long
        lib.rgpu_pdf_batch_samples.argtypes = [ctx]
    if hasattr(lib, "rgpu_state_spectra"):   # (absent from an older build of the library)
        lib.rgpu_spectrum_shells.restype = C.c_int
        lib.rgpu_spectrum_shells.argtypes = [ctx, C.POINTER(RgpuSpectrumSpec)]
        lib.rgpu_state_spectra.restype = C.c_int
        lib.rgpu_state_spectra.argtypes = [ctx, C.c_int, C.c_int, C.POINTER(RgpuSpectrumSpec), c_double_p]
        lib.rgpu_run_steps_spectra.restype = C.c_int
        lib.rgpu_run_steps_spectra.argtypes = [ctx, C.c_int, C.c_double, C.POINTER(C.c_int), c_double_p, c_double_p, c_double_p, C.c_int,
                                               C.c_int, C.POINTER(RgpuSpectrumSpec), C.POINTER(C.c_int), C.POINTER(C.c_int), c_double_p, c_double_p]
        lib.rgpu_spectrum_batch_samples.restype = C.c_long
        lib.rgpu_spectrum_batch_samples.argtypes = [ctx]
    if hasattr(lib, "rgpu_state_helm_spectra"):   # (absent from an older build of the library)
        lib.rgpu_helm_shells.restype = C.c_int
        lib.rgpu_helm_shells.argtypes = [ctx, C.POINTER(RgpuHelmSpec)]
        lib.rgpu_state_helm_spectra.restype = C.c_int
        lib.rgpu_state_helm_spectra.argtypes = [ctx, C.c_int, C.c_int, C.POINTER(RgpuHelmSpec), c_double_p]
        lib.rgpu_run_steps_helm_spectra.restype = C.c_int
        lib.rgpu_run_steps_helm_spectra.argtypes = [ctx, C.c_int, C.c_double, C.POINTER(C.c_int), c_double_p, c_double_p, c_double_p, C.c_int,
                                                    C.c_int, C.POINTER(RgpuHelmSpec), C.POINTER(C.c_int), C.POINTER(C.c_int), c_double_p, c_double_p]
        lib.rgpu_helm_batch_samples.restype = C.c_long
        lib.rgpu_helm_batch_samples.argtypes = [ctx]
    return lib


def declare_ensemble_api(lib):
    """prototypes of the rgpu_ensemble_* entry points (include/rgpu.h, "ensembles of 2D boxes")"""
    P = C.POINTER(RgpuParams)
    ens = C.c_void_p
    int_p = C.POINTER(C.c_int)
    lib.rgpu_ensemble_create.restype = C.c_int
    lib.rgpu_ensemble_create.argtypes = [P, C.c_int, C.POINTER(ens)]
    if hasattr(lib, "rgpu_ensemble_create_scan"):   # (absent from an older build of the library: scripts/ensemble_bench.py --baseline-lib)
        lib.rgpu_ensemble_create_scan.restype = C.c_int        # P: an array of `members` parameter sets
        lib.rgpu_ensemble_create_scan.argtypes = [P, C.c_int, C.POINTER(ens)]
        lib.rgpu_ensemble_scan_device_bytes.restype = C.c_size_t
        lib.rgpu_ensemble_scan_device_bytes.argtypes = [P, C.c_int]
    lib.rgpu_ensemble_destroy.restype = None
    lib.rgpu_ensemble_destroy.argtypes = [ens]
    lib.rgpu_ensemble_members.restype = C.c_int
    lib.rgpu_ensemble_members.argtypes = [ens]
    lib.rgpu_ensemble_member.restype = C.c_void_p
    lib.rgpu_ensemble_member.argtypes = [ens, C.c_int]
    lib.rgpu_ensemble_device_bytes.restype = C.c_size_t
    lib.rgpu_ensemble_device_bytes.argtypes = [P, C.c_int]
    lib.rgpu_ensemble_last_error.restype = C.c_char_p
    lib.rgpu_ensemble_last_error.argtypes = [ens]
    lib.rgpu_ensemble_run_steps.restype = C.c_int
    lib.rgpu_ensemble_run_steps.argtypes = [ens, C.c_int, c_double_p, int_p, c_double_p, c_double_p, c_double_p, int_p, int_p, int_p]
    lib.rgpu_ensemble_monitor.restype = C.c_int
    lib.rgpu_ensemble_monitor.argtypes = [ens, c_double_p]
    lib.rgpu_ensemble_run_steps_monitored.restype = C.c_int
    lib.rgpu_ensemble_run_steps_monitored.argtypes = [ens, C.c_int, c_double_p, int_p, c_double_p, c_double_p, c_double_p, int_p, int_p, int_p,
                                                      C.c_int, int_p, int_p, c_double_p, c_double_p]
    lib.rgpu_ensemble_monitor_device_bytes.restype = C.c_size_t
    lib.rgpu_ensemble_monitor_device_bytes.argtypes = [P, C.c_int]
    return lib


# every symbol include/rgpu.h declares (checked by tests/test_abi.py against the built library)
DECLARED_SYMBOLS = [
    "rgpu_create", "rgpu_create_external", "rgpu_destroy", "rgpu_state_elems", "rgpu_device_bytes", "rgpu_last_error",
    "rgpu_upload", "rgpu_download", "rgpu_device_state", "rgpu_get_params", "rgpu_stream_handle", "rgpu_inv_dt_device_slot", "rgpu_make_boundaries", "rgpu_make_boundaries_shear",
    "rgpu_make_all_boundaries", "rgpu_history_columns", "rgpu_history_reynolds", "rgpu_history_mri", "rgpu_history_turbulence", "rgpu_history_turbulence_sums", "rgpu_state_checksum", "rgpu_read_cell", "rgpu_compute_inv_dt", "rgpu_invalidate_dt", "rgpu_compute_dt", "rgpu_godunov_unsplit", "rgpu_step_pre",
    "rgpu_step_core", "rgpu_step_dissipative", "rgpu_step_core_planes", "rgpu_step_core_planes_split", "rgpu_inv_dt_fused_commit", "rgpu_inv_dt_fused_active", "rgpu_inv_dt_fusable", "rgpu_step_fill_planes", "rgpu_step_core_planes_pair", "rgpu_step_fill_planes_pair", "rgpu_inv_dt_accumulate", "rgpu_inv_dt_result",
    "rgpu_step_post_a", "rgpu_step_post_b", "rgpu_one_step_integration", "rgpu_run_steps", "rgpu_run_steps_log", "rgpu_run_steps_history", "rgpu_history_batch_heads", "rgpu_forcing_batch_steps", "rgpu_device_time_step_ready", "rgpu_clock_capable", "rgpu_clock_open", "rgpu_clock_tick", "rgpu_clock_close", "rgpu_clock_stopped", "rgpu_clock_check", "rgpu_set_option", "rgpu_get_option", "rgpu_synchronize",
    "rgpu_enable_timers", "rgpu_get_timers", "rgpu_reset_timers", "rgpu_timer_name", "rgpu_dominant_kernel",
    "rgpu_backend_name", "rgpu_arithmetic", "rgpu_selftest_arith", "rgpu_selftest_alfven", "rgpu_step_ou_forcing", "rgpu_ou_forcing_state", "rgpu_ou_forcing_get_state", "rgpu_ou_forcing_set_state", "rgpuh_params_from_ini", "rgpuh_run_settings", "rgpuh_init_condition", "rgpuh_init_gravity", "rgpu_set_gravity_field", "rgpuh_init_forcing", "rgpu_set_forcing_field", "rgpu_forcing_sums", "rgpu_add_forcing", "rgpuh_run", "rgpuh_run_hooked",
    "rgpu_ensemble_create", "rgpu_ensemble_destroy", "rgpu_ensemble_members", "rgpu_ensemble_member", "rgpu_ensemble_device_bytes", "rgpu_ensemble_last_error", "rgpu_ensemble_run_steps",
    "rgpu_ensemble_create_scan", "rgpu_ensemble_scan_device_bytes",
    "rgpu_state_monitor", "rgpu_ensemble_monitor", "rgpu_ensemble_run_steps_monitored", "rgpu_ensemble_monitor_device_bytes",
    "rgpu_state_monitor3d", "rgpu_run_steps_monitored", "rgpu_monitor_batch_samples",
    "rgpu_state_monitor_planes", "rgpu_run_steps_monitored_planes", "rgpu_monitor_planes_batch_samples",
    "rgpu_map_doubles", "rgpu_state_maps", "rgpu_run_steps_mapped", "rgpu_map_batch_samples",
    "rgpu_pdf_words", "rgpu_state_pdfs", "rgpu_run_steps_pdfs", "rgpu_pdf_batch_samples",
    "rgpu_spectrum_shells", "rgpu_state_spectra", "rgpu_run_steps_spectra", "rgpu_spectrum_batch_samples",
    "rgpu_helm_shells", "rgpu_state_helm_spectra", "rgpu_run_steps_helm_spectra", "rgpu_helm_batch_samples",
]
