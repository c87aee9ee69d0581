"""lowthrustopt_amd -- MI355X-native multiple-shooting segment propagator for low-thrust CRTBP
trajectories: the defectCalc / jacobianCalc hot path of travelingspaceman/LowThrustOpt behind a C ABI
(include/lto.h, liblto_hip.so) with a host-side mirror of the reference's closures."""
from .constants import MU, DU, TU, day, RK4, RKF78_FIXED, RKF78_ADAPTIVE, DOP853_ADAPTIVE  # noqa: F401
from ._lib import LtoError, LtoParams, LtoIntegrator, LtoDirectParams, LtoDirectTargets, LtoDirectOrbits, LtoDirectEndModel, LtoDirectTfBounds, load_library, LIB_PATH  # noqa: F401
from .hotpath import (Context, Group, Comm, GroupComm, auto_kernel, default_context, integrator, make_params, indirect_defectCalc, indirect_stm,  # noqa: F401
                      indirect_scatter, indirect_scatter_mass, indirect_jacobianCalc, direct_defectCalc, direct_jacobian_blocks,
                      direct_scatter, direct_jacobianCalc, direct_endpoint_partials, direct_midpoints, densify, indirect_newton_step, indirect_solve, indirect_solve_batch, IndirectPlan, DirectPlan, pack_soa, unpack_soa,
                      defect_norms, trial_points, line_search_pick, read_scalars, segment_order, step_stats, current_stream_ptr, direct_targets,
                      direct_qp_step, direct_solve, direct_costates, costate_scale, DirectOrbits, direct_end_model, direct_end_states,
                      direct_qp_step_free, direct_solve_free, direct_tf_bounds, direct_qp_step_free_tf, direct_solve_free_tf,
                      indirect_add_time, indirect_remesh, direct_refine, direct_resample, stack_guess, StackGuess, indirect_events, ThrustEvents,
                      indirect_events_mass, densify_mass, indirect_remesh_mass, indirect_add_time_mass, control_replay, ControlReplay,
                      replay_sample_knots, guidance_gains, GuidanceGains, guided_flight, GuidedFlight, guided_updates,
                      guidance_gains_mass, guided_flight_mass, guidance_covariance, GuidanceCovariance, halo_correct, HaloCorrect, halo_table, HaloTable,
                      HALO_HOLD_Z0, HALO_HOLD_X0, HALO_PLANAR, manifold_seeds, ManifoldSeeds, section_flight, SectionFlight,
                      state_match, StateMatch, halo_target, HaloTarget, HALO_TARGET_JACOBI, HALO_TARGET_PERIOD,
                      halo_arclength, HaloArclength, stationkeep_gains, StationkeepGains, stationkeep_flight, StationkeepFlight,
                      halo_stm, HaloStm, stationkeep_target_gains, StationkeepTargetGains)
from . import synth  # noqa: F401

__version__ = "0.1.0"
