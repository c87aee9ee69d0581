# LowThrustOptHIP.jl -- Julia binding of liblto_hip.so (include/lto.h) for LowThrustOpt's shooting drivers.
#
# What it replaces: the bodies of the four closures nested in the reference drivers
#   multiShoot_CRTBP_indirect:  defectCalc (src/multiShoot_CRTBP_indirect.jl:63-90), jacobianCalc (:93-146)
#   multiShoot_CRTBP_direct:    defectCalc (src/multiShoot_CRTBP_direct.jl:66-109),  jacobianCalc (:111-166),
#                               tf partial (:503-516)
# The drivers' signatures, return tuples and inner array shapes are unchanged (INTEGRATION.md shows the patch).
#
# STATUS: there is no `julia` binary in the build image or on the GPU box, so this file has never been
# executed.  It is kept deliberately thin: every ccall below has a line-for-line twin in
# lowthrustopt_amd/_lib.py + hotpath.py (ctypes), and THAT twin is what the test-suite drives on the GPU.
module LowThrustOptHIP

using SparseArrays, LinearAlgebra, Libdl

export LtoIndirectPlan, LtoDirectPlan, LtoComm, LtoCommWindows, pinned_array, pack_soa!, unpack_soa!, defect_norms!, indirect_defect_dev!,
       indirect_jacobian_dev!, newton_solve_dev!, axpy_dev!, direct_defect_dev!, direct_jacobian_dev!, rebalance!, set_kernel!, set_warm_start!, set_defect_lanes!,
       comm_unique_id, allgather_dev!, allreduce_dev!, ctx_stream, last_call_ms, copy_order!, segment_order_dev!, step_stats_dev!
export LtoContext, LtoGroup, indirect_defectCalc, indirect_jacobianCalc, indirect_stm, indirect_newton_step, indirect_solve, indirect_solve_batch, densify, densify_mass, addTimeFinal, tf_sweep, addTimeFinal_mass, tf_sweep_mass, meshRefine_indirect, remesh_batch, meshRefine_indirect_mass, remesh_mass_batch,
       direct_defectCalc, direct_jacobianCalc, direct_midpoints, direct_refine, direct_resample, direct_qp_step, direct_solve, direct_costates, direct_end_states, direct_qp_step_free, direct_solve_free, stack_guess, halo_correct, halo_target, halo_arclength, halo_table, manifold_seeds, section_flight, state_match, stationkeep_gains, stationkeep_flight, halo_stm, stationkeep_target_gains,
       LtoDirectTfBounds, direct_qp_step_free_tf, direct_solve_free_tf, guidance_gains, guided_flight, guidance_gains_mass, guided_flight_mass, guidance_covariance,
       LtoDirectTargets, LtoDirectEndModel, LTO_RK4, LTO_RKF78_FIXED, LTO_RKF78_ADAPTIVE, LTO_DOP853_ADAPTIVE

const liblto = get(ENV, "LTO_HIP_LIB", joinpath(@__DIR__, "..", "lowthrustopt_amd", "liblto_hip.so"))

const LTO_RK4 = Cint(0)
const LTO_RKF78_FIXED = Cint(1)
const LTO_RKF78_ADAPTIVE = Cint(2)
const LTO_DOP853_ADAPTIVE = Cint(3)
# error codes (include/lto.h): < 0 = misuse, > 0 = run time
const LTO_EINVAL, LTO_ENULL, LTO_EUNSUPPORTED = Cint(-1), Cint(-2), Cint(-3)
const LTO_EHIP, LTO_EBADP, LTO_ENODEVICE, LTO_ENOMEM = Cint(1), Cint(2), Cint(3), Cint(4)
# kernel families of an indirect plan's STM sweep (lto_indirect_plan_set_kernel; 0 = let the library choose)
const LTO_KERNEL_AUTO, LTO_KERNEL_PER_LANE, LTO_KERNEL_COOP, LTO_KERNEL_DIRECT_PIPE = Cint(0), Cint(1), Cint(2), Cint(3)
const LTO_KERNEL_PIPE8, LTO_KERNEL_COOP2, LTO_KERNEL_PIPE48, LTO_KERNEL_PIPE32, LTO_KERNEL_LANE = Cint(5), Cint(6), Cint(7), Cint(8), Cint(9)
const LTO_LAYOUT_SOA, LTO_LAYOUT_BLOCKS = Cint(0), Cint(1)

# isbits mirrors of the C structs (include/lto.h)
struct LtoIntegrator
    method::Cint
    steps::Cint
    rtol::Cdouble
    atol::Cdouble
    max_steps::Cint
end
# default = the reference's Vern8() setting: adaptive order-8 pair, reltol = abstol = 1e-13 (indirect.jl:79)
LtoIntegrator() = LtoIntegrator(LTO_DOP853_ADAPTIVE, 0, 1e-13, 1e-13, 0)

struct LtoParams          # the `params` tuple of indirect.jl:260, field for field
    MU::Cdouble; DU::Cdouble; TU::Cdouble; thrustLimit::Cdouble
    mass::Cdouble; time_direction::Cdouble; p::Cdouble; rho::Cdouble
end
LtoParams(t::Tuple) = LtoParams(map(Float64, t)...)

struct LtoDirectParams
    MU::Cdouble; DU::Cdouble; TU::Cdouble; Isp::Cdouble
end

# per-trajectory targets of the direct QP step (lto_direct_targets): interpolated end states, initial mass, current impulses
struct LtoDirectTargets
    s0::NTuple{6,Cdouble}; sf::NTuple{6,Cdouble}; mass::Cdouble; dV1::NTuple{3,Cdouble}; dV2::NTuple{3,Cdouble}
end
LtoDirectTargets(s0, sf, mass, dV1, dV2) = LtoDirectTargets(NTuple{6,Cdouble}(s0), NTuple{6,Cdouble}(sf), Cdouble(mass),
                                                            NTuple{3,Cdouble}(dV1), NTuple{3,Cdouble}(dV2))

# the two orbit tables of the free-end model (lto_direct_orbits): the arrays must stay alive across the call (GC.@preserve)
struct LtoDirectOrbits
    n0::Cint; nf::Cint; t0::Ptr{Cdouble}; X0::Ptr{Cdouble}; tf::Ptr{Cdouble}; Xf::Ptr{Cdouble}
end
# per-trajectory end model of a free-end step (lto_direct_end_model)
struct LtoDirectEndModel
    g0::NTuple{6,Cdouble}; gf::NTuple{6,Cdouble}; c0_norm::Cdouble; cf_norm::Cdouble
end
LtoDirectEndModel(g0, gf, c0, cf) = LtoDirectEndModel(NTuple{6,Cdouble}(g0), NTuple{6,Cdouble}(gf), Cdouble(c0), Cdouble(cf))

mutable struct LtoContext
    handle::Ptr{Cvoid}
    function LtoContext(device::Integer = 0)
        h = Ref{Ptr{Cvoid}}(C_NULL)
        rc = ccall((:lto_create, liblto), Cint, (Ref{Ptr{Cvoid}}, Cint), h, device)
        rc == 0 || error("lto_create failed with code $rc (no gfx950 device?)")
        ctx = new(h[])
        finalizer(c -> (c.handle == C_NULL || ccall((:lto_destroy, liblto), Cvoid, (Ptr{Cvoid},), c.handle); c.handle = C_NULL), ctx)
        ctx
    end
end

"""Several GPUs behind this one Julia process (lto_group_*, include/lto.h): `LtoGroup([0, 1, 2, 3])`.  Accepted wherever
the four sweep closures take an `LtoContext`; each sweep is split into contiguous shards (segment blocks with a
one-node halo, or whole trajectories of a batch), one host thread and one device context per entry."""
mutable struct LtoGroup
    handle::Ptr{Cvoid}
    function LtoGroup(devices::Vector{<:Integer})
        h = Ref{Ptr{Cvoid}}(C_NULL)
        ids = Cint.(devices)
        rc = ccall((:lto_group_create, liblto), Cint, (Cint, Ptr{Cint}, Ref{Ptr{Cvoid}}), length(ids), ids, h)
        rc == 0 || error("lto_group_create failed with code $rc")
        g = new(h[])
        finalizer(c -> (c.handle == C_NULL || ccall((:lto_group_destroy, liblto), Cvoid, (Ptr{Cvoid},), c.handle); c.handle = C_NULL), g)
        g
    end
end

const LtoHandle = Union{LtoContext, LtoGroup}
const _libhandle = Ref{Ptr{Cvoid}}(C_NULL)
libhandle() = (_libhandle[] == C_NULL && (_libhandle[] = Libdl.dlopen(liblto)); _libhandle[])
# entry point of a sweep: lto_<name> for one context, lto_group_<name> for a group (identical argument lists)
entry(::LtoContext, name::Symbol) = Libdl.dlsym(libhandle(), Symbol("lto_", name))
entry(::LtoGroup, name::Symbol) = Libdl.dlsym(libhandle(), Symbol("lto_group_", name))
last_error(ctx::LtoContext) = unsafe_string(ccall((:lto_last_error, liblto), Cstring, (Ptr{Cvoid},), ctx.handle))
last_error(g::LtoGroup) = unsafe_string(ccall((:lto_group_last_error, liblto), Cstring, (Ptr{Cvoid},), g.handle))

function check(ctx::LtoHandle, rc::Cint)
    rc == 0 && return
    msg = last_error(ctx)
    # code 2 is the reference's own error("Invalid value of p!") (CRTBP_stateCostate_deriv.jl:52); code 4 = host memory / threads ran out inside the call
    rc == LTO_ENOMEM && throw(OutOfMemoryError())
    error(rc == LTO_EBADP ? msg : "lto error $rc: $msg")
end

# ---------------------------------------------------------------------------------------------- indirect
"defectCalc of multiShoot_CRTBP_indirect: returns (defect1[2nstate x (n_nodes-1)], errors[n_nodes-1])."
function indirect_defectCalc(ctx::LtoHandle, XC_all::Matrix{Float64}, t_TU::Vector{Float64}, params;
                             integ::LtoIntegrator = LtoIntegrator())
    ndim, n_nodes = size(XC_all)
    defect1 = zeros(ndim, n_nodes - 1)
    errors = zeros(n_nodes - 1)
    prm = Ref(LtoParams(params))
    rc = ccall(entry(ctx, :indirect_defect), Cint,
               (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ref{LtoParams}, Cint, Ref{LtoIntegrator},
                Ptr{Cdouble}, Ptr{Cdouble}),
               ctx.handle, ndim, n_nodes, 1, XC_all, t_TU, 1, prm, 1, Ref(integ), defect1, errors)
    check(ctx, rc)
    (defect1, errors)
end

"Compact Jacobian blocks Phi[2nstate x 2nstate x (n_nodes-1)] (= ForwardDiff.jacobian(f, x0) of indirect.jl:121) and the defect."
function indirect_stm(ctx::LtoHandle, XC_all::Matrix{Float64}, t_TU::Vector{Float64}, params;
                      integ::LtoIntegrator = LtoIntegrator())
    ndim, n_nodes = size(XC_all)
    Phi = zeros(ndim, ndim, n_nodes - 1)
    defect1 = zeros(ndim, n_nodes - 1)
    prm = Ref(LtoParams(params))
    rc = ccall(entry(ctx, :indirect_jacobian), Cint,
               (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ref{LtoParams}, Cint, Ref{LtoIntegrator},
                Ptr{Cdouble}, Ptr{Cdouble}),
               ctx.handle, ndim, n_nodes, 1, XC_all, t_TU, 1, prm, 1, Ref(integ), Phi, defect1)
    check(ctx, rc)
    (Phi, defect1)
end

"""jacobianCalc of multiShoot_CRTBP_indirect: Jac_full [2nstate(n_nodes-1) x 2nstate*n_nodes], row block i =
[Phi_i | -I] at columns 2nstate(i-1)+(1:4nstate), with the columns of the two fixed end states zeroed
(indirect.jl:123-142).  Returned sparse: the driver's least-squares step sparsifies it anyway (:181)."""
function indirect_jacobianCalc(ctx::LtoHandle, XC_all, t_TU, nstate, n_nodes, params; integ = LtoIntegrator())
    (Phi, _) = indirect_stm(ctx, XC_all, t_TU, params; integ = integ)
    nd = 2 * nstate
    S = n_nodes - 1
    I_idx = Int[]; J_idx = Int[]; V = Float64[]
    for i = 1:S, c = 1:nd, r = 1:nd
        push!(I_idx, (i - 1) * nd + r); push!(J_idx, (i - 1) * nd + c); push!(V, Phi[r, c, i])
    end
    for i = 1:S, r = 1:nd
        push!(I_idx, (i - 1) * nd + r); push!(J_idx, i * nd + r); push!(V, -1.0)
    end
    Jac_full = sparse(I_idx, J_idx, V, nd * S, nd * n_nodes)
    Jac_full[:, 1:nstate] .= 0
    Jac_full[:, (nd * n_nodes - 2 * nstate + 1):(nd * n_nodes - nstate)] .= 0
    dropzeros!(Jac_full)
end

"""One Newton iteration on the device (indirect.jl:290-296): jacobianCalc, the least-squares step of
optimizeTraj_OLS (incl. the flag_adjointsOnly column mask) and its second-order correction; returns (xc_update, defect).
12 or 14 rows; for 14 the pinned entries are those of `indirect_solve`."""
function indirect_newton_step(ctx::LtoContext, XC_all::Matrix{Float64}, t_TU::Vector{Float64}, params;
                              integ::LtoIntegrator = LtoIntegrator(), flag_adjointsOnly::Bool = false,
                              soc_threshold::Float64 = 1e-1)
    ndim, n_nodes = size(XC_all)
    xc_update = zeros(ndim, n_nodes)
    defect1 = zeros(ndim, n_nodes - 1)
    rc = ccall((:lto_indirect_newton_step, liblto), Cint,
               (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ref{LtoParams}, Cint, Ref{LtoIntegrator},
                Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}),
               ctx.handle, ndim, n_nodes, 1, XC_all, t_TU, 1, Ref(LtoParams(params)), 1, Ref(integ),
               flag_adjointsOnly ? 1 : 0, soc_threshold, xc_update, defect1)
    check(ctx, rc)
    (xc_update, defect1)
end

"densify (src/HelperFunctions.jl:51-101): (XC_dense[ndim x n_desired], t_dense)."
function densify(ctx::LtoContext, XC_all::Matrix{Float64}, t_TU::Vector{Float64}, params, n_desired::Integer;
                 integ::LtoIntegrator = LtoIntegrator())
    ndim, n_nodes = size(XC_all)
    XC_dense = zeros(ndim, n_desired)
    t_dense = zeros(n_desired)
    rc = ccall((:lto_indirect_densify, liblto), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ref{LtoParams}, Ref{LtoIntegrator}, Cint, Ptr{Cdouble},
                Ptr{Cdouble}),
               ctx.handle, ndim, n_nodes, XC_all, t_TU, Ref(LtoParams(params)), Ref(integ), n_desired, XC_dense, t_dense)
    check(ctx, rc)
    (XC_dense, t_dense)
end

"""densify for one solution of the 14-row variable-mass system (`lto_indirect_densify_mass`, DESIGN 4.20): `XC_all` [14 x n_nodes],
`params` with Isp in the mass slot.  Returns (XC_dense [14 x n_desired], t_dense); row 7 is the propagated mass."""
function densify_mass(ctx::LtoContext, XC_all::Matrix{Float64}, t_TU::Vector{Float64}, params, n_desired::Integer;
                      integ::LtoIntegrator = LtoIntegrator())
    size(XC_all, 1) == 14 || throw(ArgumentError("densify_mass takes the 14-row solution [14 x n_nodes]"))
    n_nodes = size(XC_all, 2)
    XC_dense = zeros(14, n_desired)
    t_dense = zeros(n_desired)
    rc = ccall((:lto_indirect_densify_mass, liblto), Cint,
               (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ref{LtoParams}, Ref{LtoIntegrator}, Cint, Ptr{Cdouble}, Ptr{Cdouble}),
               ctx.handle, n_nodes, XC_all, t_TU, Ref(LtoParams(params)), Ref(integ), n_desired, XC_dense, t_dense)
    check(ctx, rc)
    (XC_dense, t_dense)
end

"""The whole Newton loop of multiShoot_CRTBP_indirect (indirect.jl:254-345) in one library call, trajectory resident on
the GPU: returns (XC_all, defect, status_flag) exactly as the reference driver does, so
`multiShoot_CRTBP_indirect(XC_all, t_TU, MU, DU, TU, n_nodes, mass0, thrustLimit, plot_yn, flag_adjointsOnly, maxIter, p, rho)`
can forward to `indirect_solve(LTO, XC_all, t_TU, (MU, DU, TU, thrustLimit, mass0, 1.0, p, rho), flag_adjointsOnly, maxIter)`
when `plot_yn` is false.  14 rows (r, v, m, λ_r, λ_v, λ_m; Isp in the tuple's mass slot) solve the variable-mass system with a
free final mass: XC_all[1:7, 1], XC_all[1:6, end] and XC_all[14, end] = λ_m(tf) = 0 are pinned (the last is set on entry)."""
function indirect_solve(ctx::LtoContext, XC_all::Matrix{Float64}, t_TU::Vector{Float64}, params, flag_adjointsOnly::Bool,
                        maxIter::Integer; integ::LtoIntegrator = LtoIntegrator(), verbose::Bool = true)
    ndim, n_nodes = size(XC_all)
    XC_new = zeros(ndim, n_nodes)
    defect1 = zeros(ndim, n_nodes - 1)
    history = fill(NaN, 2, max(maxIter, 1))
    status = Ref{Cint}(0); iters = Ref{Cint}(0)
    rc = ccall((:lto_indirect_solve, liblto), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ref{LtoParams}, Ref{LtoIntegrator}, Cint, Cint,
                Ptr{Cdouble}, Ptr{Cdouble}, Ref{Cint}, Ref{Cint}, Ptr{Cdouble}),
               ctx.handle, ndim, n_nodes, XC_all, t_TU, Ref(LtoParams(params)), Ref(integ), flag_adjointsOnly ? 1 : 0, maxIter,
               XC_new, defect1, status, iters, history)
    check(ctx, rc)
    if verbose
        for k = 1:size(history, 2)
            isnan(history[2, k]) && break
            println("Iter $k. Max defect = $(history[1, k]). α = $(history[2, k]).")
        end
        status[] == 1 && println("Reached max iteration count at $(iters[]) iterations")
    end
    (XC_new, defect1, Int(status[]))
end

"""n_batch independent Newton loops side by side (`lto_indirect_solve_batch`): `XC_all` [12 or 14 x n_nodes x n_batch], `t_TU`
[n_nodes] (shared grid), `params` a vector of n_batch parameter tuples (e.g. one rho per level of a continuation ladder).
Returns (XC_all, defect, status_flags, iterCounts)."""
function indirect_solve_batch(ctx::LtoContext, XC_all::Array{Float64,3}, t_TU::Vector{Float64}, params::Vector,
                              flag_adjointsOnly::Bool, maxIter::Integer; integ::LtoIntegrator = LtoIntegrator())
    ndim, n_nodes, n_batch = size(XC_all)
    prm = [LtoParams(q) for q in params]
    XC_new = zeros(ndim, n_nodes, n_batch)
    defect1 = zeros(ndim, n_nodes - 1, n_batch)
    status = zeros(Cint, n_batch); iters = zeros(Cint, n_batch)
    rc = ccall((:lto_indirect_solve_batch, liblto), Cint,
               (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{LtoParams}, Cint, Ref{LtoIntegrator}, Cint, Cint,
                Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}),
               ctx.handle, ndim, n_nodes, n_batch, XC_all, t_TU, 1, prm, length(prm), Ref(integ), flag_adjointsOnly ? 1 : 0, maxIter,
               XC_new, defect1, status, iters, C_NULL)
    check(ctx, rc)
    (XC_new, defect1, Int.(status), Int.(iters))
end

"""addTimeFinal (src/HelperFunctions.jl:196-250, re-specified: DESIGN 4.12) in one library call (`lto_indirect_add_time`): the
converged 12-row solution with a ballistic tail of Δt TU, densified at `n_desired` points, re-meshed onto LinRange(t[1], t[end] + Δt,
n_nodes), its end snapped onto the arrival table (`Xf_times` in [0, 1], `Xf_states` [6 x nf]) and re-solved with fixed ends.
Returns (XC_new, t_new) on status 0, otherwise the original (XC_all, t_TU) -- the reference's convention (:239-249)."""
function addTimeFinal(ctx::LtoContext, XC_all::Matrix{Float64}, t_TU::Vector{Float64}, Δt, MU, DU, TU, n_nodes, mass, thrustLimit,
                      p, rho, Xf_times::Vector{Float64}, Xf_states::Matrix{Float64}; maxIter::Integer = 10, n_desired::Integer = 200,
                      flag_adjointsOnly::Bool = false, integ::LtoIntegrator = LtoIntegrator())
    ndim = size(XC_all, 1)
    XC_new = zeros(ndim, n_nodes); t_new = zeros(n_nodes); tau = zeros(1); defect1 = zeros(ndim, n_nodes - 1)
    status = Ref{Cint}(0); iters = Ref{Cint}(0)
    prm = Ref(LtoParams((MU, DU, TU, thrustLimit, mass, 1.0, p, rho)))
    rc = GC.@preserve Xf_times Xf_states begin
        ob = Ref(LtoDirectOrbits(0, length(Xf_times), C_NULL, C_NULL, pointer(Xf_times), pointer(Xf_states)))
        ccall((:lto_indirect_add_time, liblto), Cint,
              (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ref{LtoParams}, Ref{LtoIntegrator}, Ref{LtoDirectOrbits}, Cdouble,
               Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint},
               Ptr{Cdouble}, Ptr{Cdouble}),
              ctx.handle, ndim, n_nodes, XC_all, t_TU, prm, Ref(integ), ob, Float64(Δt), n_desired, flag_adjointsOnly ? 1 : 0,
              maxIter, C_NULL, XC_new, t_new, tau, defect1, status, iters, C_NULL, C_NULL)
    end
    check(ctx, rc)
    status[] == 0 ? (XC_new, t_new) : (XC_all, t_TU)
end

"""addTimeFinal for many Δt side by side (`lto_indirect_add_time_batch`): the cost-versus-time-of-flight curve of a converged
transfer.  Returns (XC [12 x n x K], t [n x K], tau [K], status [K], iterations [K], cost [K] in DU/TU)."""
function tf_sweep(ctx::LtoContext, XC_all::Matrix{Float64}, t_TU::Vector{Float64}, Δts::Vector{Float64}, MU, DU, TU, mass,
                  thrustLimit, p, rho, Xf_times::Vector{Float64}, Xf_states::Matrix{Float64}; maxIter::Integer = 10,
                  n_desired::Integer = 200, flag_adjointsOnly::Bool = false, integ::LtoIntegrator = LtoIntegrator())
    ndim, n_nodes = size(XC_all)
    K = length(Δts)
    XC = zeros(ndim, n_nodes, K); t = zeros(n_nodes, K); tau = zeros(K); defect1 = zeros(ndim, n_nodes - 1, K)
    status = zeros(Cint, K); iters = zeros(Cint, K); cost = zeros(K)
    prm = Ref(LtoParams((MU, DU, TU, thrustLimit, mass, 1.0, p, rho)))
    rc = GC.@preserve Xf_times Xf_states begin
        ob = Ref(LtoDirectOrbits(0, length(Xf_times), C_NULL, C_NULL, pointer(Xf_times), pointer(Xf_states)))
        ccall((:lto_indirect_add_time_batch, liblto), Cint,
              (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ref{LtoParams}, Ref{LtoIntegrator}, Ref{LtoDirectOrbits}, Cint,
               Ptr{Cdouble}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint},
               Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}),
              ctx.handle, ndim, n_nodes, XC_all, t_TU, prm, Ref(integ), ob, K, Δts, n_desired, flag_adjointsOnly ? 1 : 0, maxIter,
              C_NULL, XC, t, tau, defect1, status, iters, C_NULL, cost)
    end
    check(ctx, rc)
    (XC, t, tau, Int.(status), Int.(iters), cost)
end

"""addTimeFinal for a converged solution of the 14-row variable-mass system (`lto_indirect_add_time_mass`, DESIGN 4.21): `XC_all`
[14 x n_nodes], Isp in the mass slot of the parameters.  Rows 8:14 of the last node are zeroed on a copy; the tail of Δt TU is the
14-row system's own flow with zero costates (the orbit coasts; the mass follows the law's flow at |λ_v| = 0: constant for p > 1,
full throttle for p = 0, the idle flow aL / (1 + e^(1/ρ)) for p = 1); the 14-row loop re-solves with r0, v0, m0 and rf, vf fixed and
the final mass free.  Returns (XC_new, t_new) on status 0, otherwise the original (XC_all, t_TU)."""
function addTimeFinal_mass(ctx::LtoContext, XC_all::Matrix{Float64}, t_TU::Vector{Float64}, Δt, MU, DU, TU, n_nodes, Isp, thrustLimit,
                           p, rho, Xf_times::Vector{Float64}, Xf_states::Matrix{Float64}; maxIter::Integer = 10,
                           n_desired::Integer = 200, flag_adjointsOnly::Bool = false, integ::LtoIntegrator = LtoIntegrator())
    size(XC_all) == (14, n_nodes) || throw(ArgumentError("addTimeFinal_mass takes the 14-row solution [14 x n_nodes]"))
    XC_new = zeros(14, n_nodes); t_new = zeros(n_nodes); tau = zeros(1); defect1 = zeros(14, n_nodes - 1)
    status = Ref{Cint}(0); iters = Ref{Cint}(0)
    prm = Ref(LtoParams((MU, DU, TU, thrustLimit, Isp, 1.0, p, rho)))
    rc = GC.@preserve Xf_times Xf_states begin
        ob = Ref(LtoDirectOrbits(0, length(Xf_times), C_NULL, C_NULL, pointer(Xf_times), pointer(Xf_states)))
        ccall((:lto_indirect_add_time_mass, liblto), Cint,
              (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ref{LtoParams}, Ref{LtoIntegrator}, Ref{LtoDirectOrbits}, Cdouble,
               Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint},
               Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
              ctx.handle, n_nodes, XC_all, t_TU, prm, Ref(integ), ob, Float64(Δt), n_desired, flag_adjointsOnly ? 1 : 0,
              maxIter, C_NULL, XC_new, t_new, tau, defect1, status, iters, C_NULL, C_NULL, C_NULL)
    end
    check(ctx, rc)
    status[] == 0 ? (XC_new, t_new) : (XC_all, t_TU)
end

"""addTimeFinal_mass for many Δt side by side (`lto_indirect_add_time_mass_batch`): the propellant-versus-time-of-flight curve of a
converged variable-mass transfer.  Returns (XC [14 x n x K], t [n x K], tau [K], status [K], iterations [K], cost [K] in DU/TU,
propellant [K] in kg = XC_all[7, 1] - XC[7, end, k])."""
function tf_sweep_mass(ctx::LtoContext, XC_all::Matrix{Float64}, t_TU::Vector{Float64}, Δts::Vector{Float64}, MU, DU, TU, Isp,
                       thrustLimit, p, rho, Xf_times::Vector{Float64}, Xf_states::Matrix{Float64}; maxIter::Integer = 10,
                       n_desired::Integer = 200, flag_adjointsOnly::Bool = false, integ::LtoIntegrator = LtoIntegrator())
    size(XC_all, 1) == 14 || throw(ArgumentError("tf_sweep_mass takes the 14-row solution [14 x n_nodes]"))
    n_nodes = size(XC_all, 2)
    K = length(Δts)
    XC = zeros(14, n_nodes, K); t = zeros(n_nodes, K); tau = zeros(K); defect1 = zeros(14, n_nodes - 1, K)
    status = zeros(Cint, K); iters = zeros(Cint, K); cost = zeros(K); propellant = zeros(K)
    prm = Ref(LtoParams((MU, DU, TU, thrustLimit, Isp, 1.0, p, rho)))
    rc = GC.@preserve Xf_times Xf_states begin
        ob = Ref(LtoDirectOrbits(0, length(Xf_times), C_NULL, C_NULL, pointer(Xf_times), pointer(Xf_states)))
        ccall((:lto_indirect_add_time_mass_batch, liblto), Cint,
              (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ref{LtoParams}, Ref{LtoIntegrator}, Ref{LtoDirectOrbits}, Cint,
               Ptr{Cdouble}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint},
               Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
              ctx.handle, n_nodes, XC_all, t_TU, prm, Ref(integ), ob, K, Δts, n_desired, flag_adjointsOnly ? 1 : 0, maxIter,
              C_NULL, XC, t, tau, defect1, status, iters, C_NULL, cost, propellant)
    end
    check(ctx, rc)
    (XC, t, tau, Int.(status), Int.(iters), cost, propellant)
end

"""Mesh re-distribution of a converged 12-row indirect solution (`lto_indirect_remesh`, DESIGN 4.13), the counterpart of
meshRefine_direct: `n_new` nodes (default: as many as before) placed so that every segment takes the same share of the integrator's
trial steps (`passes` times over) or of `weights` [n_nodes - 1] (then `passes` must be 1), the new nodes taken from the solution's own
piecewise trajectory, then the fixed-end Newton loop on the new grid.  Returns (XC_new, t_new, n_new) on status 0, otherwise the
original (XC_all, t_TU, n_nodes) -- the convention of addTimeFinal."""
function meshRefine_indirect(ctx::LtoContext, XC_all::Matrix{Float64}, t_TU::Vector{Float64}, MU, DU, TU, n_nodes, mass, thrustLimit,
                             p, rho; n_new::Integer = n_nodes, passes::Integer = 2, weights::Union{Nothing,Vector{Float64}} = nothing,
                             maxIter::Integer = 10, flag_adjointsOnly::Bool = false, integ::LtoIntegrator = LtoIntegrator())
    ndim = size(XC_all, 1)
    XC_new = zeros(ndim, n_new); t_new = zeros(n_new); defect1 = zeros(ndim, n_new - 1)
    status = Ref{Cint}(0); iters = Ref{Cint}(0)
    prm = Ref(LtoParams((MU, DU, TU, thrustLimit, mass, 1.0, p, rho)))
    rc = ccall((:lto_indirect_remesh, liblto), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ref{LtoParams}, Ref{LtoIntegrator}, Cint, Ptr{Cdouble}, Cint, Cint,
                Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}),
               ctx.handle, ndim, n_nodes, XC_all, t_TU, prm, Ref(integ), n_new, weights === nothing ? C_NULL : weights, passes,
               flag_adjointsOnly ? 1 : 0, maxIter, t_new, C_NULL, XC_new, defect1, status, iters, C_NULL, C_NULL, C_NULL)
    check(ctx, rc)
    status[] == 0 ? (XC_new, t_new, Int(n_new)) : (XC_all, t_TU, Int(n_nodes))
end

"""Mesh re-distribution of n_batch solutions side by side (`lto_indirect_remesh_batch`): `XC_all` [12 x n_nodes x n_batch], `t_TU`
[n_nodes x n_batch], `params` a vector of n_batch parameter tuples.  Returns (XC [12 x n_new x B], t [n_new x B], status [B],
iterations [B], steps_before [(n_nodes-1) x B], steps_after [(n_new-1) x B])."""
function remesh_batch(ctx::LtoContext, XC_all::Array{Float64,3}, t_TU::Matrix{Float64}, params::Vector; n_new::Integer = size(XC_all, 2),
                      passes::Integer = 2, maxIter::Integer = 10, flag_adjointsOnly::Bool = false, integ::LtoIntegrator = LtoIntegrator())
    ndim, n_nodes, B = size(XC_all)
    prm = [LtoParams(q) for q in params]
    XC = zeros(ndim, n_new, B); t = zeros(n_new, B); defect1 = zeros(ndim, n_new - 1, B)
    status = zeros(Cint, B); iters = zeros(Cint, B); before = zeros(Cint, n_nodes - 1, B); after = zeros(Cint, n_new - 1, B)
    rc = ccall((:lto_indirect_remesh_batch, liblto), Cint,
               (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{LtoParams}, Cint, Ref{LtoIntegrator}, Cint,
                Ptr{Cdouble}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint},
                Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}),
               ctx.handle, ndim, n_nodes, B, XC_all, t_TU, B, prm, length(prm), Ref(integ), n_new, C_NULL, passes,
               flag_adjointsOnly ? 1 : 0, maxIter, t, C_NULL, XC, defect1, status, iters, C_NULL, before, after)
    check(ctx, rc)
    (XC, t, Int.(status), Int.(iters), Int.(before), Int.(after))
end

"""`meshRefine_indirect` for a converged solution of the 14-row variable-mass system (`lto_indirect_remesh_mass`, DESIGN 4.20):
`XC_all` [14 x n_nodes], Isp in place of the mass.  The re-solve keeps r0, v0, m0 and rf, vf and leaves the final mass free.  Returns
(XC_new, t_new, n_new) on status 0, otherwise the original (XC_all, t_TU, n_nodes)."""
function meshRefine_indirect_mass(ctx::LtoContext, XC_all::Matrix{Float64}, t_TU::Vector{Float64}, MU, DU, TU, n_nodes, Isp,
                                  thrustLimit, p, rho; n_new::Integer = n_nodes, passes::Integer = 2,
                                  weights::Union{Nothing,Vector{Float64}} = nothing, maxIter::Integer = 10,
                                  flag_adjointsOnly::Bool = false, integ::LtoIntegrator = LtoIntegrator())
    size(XC_all) == (14, n_nodes) || throw(ArgumentError("meshRefine_indirect_mass takes the 14-row solution [14 x n_nodes]"))
    length(t_TU) == n_nodes || throw(ArgumentError("meshRefine_indirect_mass takes one time per node"))
    XC_new = zeros(14, n_new); t_new = zeros(n_new); defect1 = zeros(14, n_new - 1)
    status = Ref{Cint}(0); iters = Ref{Cint}(0)
    prm = Ref(LtoParams((MU, DU, TU, thrustLimit, Isp, 1.0, p, rho)))
    rc = ccall((:lto_indirect_remesh_mass, liblto), Cint,
               (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ref{LtoParams}, Ref{LtoIntegrator}, Cint, Ptr{Cdouble}, Cint, Cint,
                Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}),
               ctx.handle, n_nodes, XC_all, t_TU, prm, Ref(integ), n_new, weights === nothing ? C_NULL : weights, passes,
               flag_adjointsOnly ? 1 : 0, maxIter, t_new, C_NULL, XC_new, defect1, status, iters, C_NULL, C_NULL, C_NULL)
    check(ctx, rc)
    status[] == 0 ? (XC_new, t_new, Int(n_new)) : (XC_all, t_TU, Int(n_nodes))
end

"""`remesh_batch` for the 14-row variable-mass system (`lto_indirect_remesh_mass_batch`): `XC_all` [14 x n_nodes x n_batch], `params`
with Isp in the mass slot.  Returns (XC [14 x n_new x B], t [n_new x B], status [B], iterations [B], steps_before, steps_after)."""
function remesh_mass_batch(ctx::LtoContext, XC_all::Array{Float64,3}, t_TU::Matrix{Float64}, params::Vector;
                           n_new::Integer = size(XC_all, 2), passes::Integer = 2, maxIter::Integer = 10,
                           flag_adjointsOnly::Bool = false, integ::LtoIntegrator = LtoIntegrator())
    ndim, n_nodes, B = size(XC_all)
    ndim == 14 || throw(ArgumentError("remesh_mass_batch takes 14-row solutions [14 x n_nodes x n_batch]"))
    prm = [LtoParams(q) for q in params]
    XC = zeros(14, n_new, B); t = zeros(n_new, B); defect1 = zeros(14, n_new - 1, B)
    status = zeros(Cint, B); iters = zeros(Cint, B); before = zeros(Cint, n_nodes - 1, B); after = zeros(Cint, n_new - 1, B)
    rc = ccall((:lto_indirect_remesh_mass_batch, liblto), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{LtoParams}, Cint, Ref{LtoIntegrator}, Cint,
                Ptr{Cdouble}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint},
                Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}),
               ctx.handle, n_nodes, B, XC_all, t_TU, B, prm, length(prm), Ref(integ), n_new, C_NULL, passes,
               flag_adjointsOnly ? 1 : 0, maxIter, t, C_NULL, XC, defect1, status, iters, C_NULL, before, after)
    check(ctx, rc)
    (XC, t, Int.(status), Int.(iters), Int.(before), Int.(after))
end

"""Switch times, burn arcs and dv of n_batch indirect solutions (`lto_indirect_events_batch`, DESIGN 4.18): `XC_all`
[12 x n_nodes x n_batch], `t_TU` [n_nodes x n_batch], `params` a vector of n_batch parameter tuples.  Per trajectory a named tuple
(arcs = [(t_on, t_off)] in TU, dv in DU/TU, burn_time in TU, n_events, status)."""
function thrust_arcs(ctx::LtoContext, XC_all::Array{Float64,3}, t_TU::Matrix{Float64}, params::Vector; max_events::Integer = 64,
                     integ::LtoIntegrator = LtoIntegrator())
    ndim, n_nodes, B = size(XC_all)
    prm = [LtoParams(q) for q in params]
    n_events = zeros(Cint, B); t_event = fill(NaN, max_events, B); kind = zeros(Cint, max_events, B); on0 = zeros(Cint, B)
    dv = zeros(B); burn = zeros(B); status = zeros(Cint, B)
    rc = ccall((:lto_indirect_events_batch, liblto), Cint,
               (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{LtoParams}, Cint, Ref{LtoIntegrator}, Cint,
                Ptr{Cint}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
               ctx.handle, ndim, n_nodes, B, XC_all, t_TU, B, prm, length(prm), Ref(integ), max_events, n_events, t_event, kind, on0,
               dv, burn, C_NULL, status)
    check(ctx, rc)
    map(1:B) do b
        arcs = Tuple{Float64,Float64}[]
        on = on0[b] != 0; mark = t_TU[1, b]
        for k in 1:min(n_events[b], max_events)
            isnan(t_event[k, b]) && break
            on ? push!(arcs, (mark, t_event[k, b])) : (mark = t_event[k, b])
            on = !on
        end
        (on && status[b] == 0) && push!(arcs, (mark, t_TU[end, b]))
        (arcs = arcs, dv = dv[b], burn_time = burn[b], n_events = Int(n_events[b]), status = Int(status[b]))
    end
end

"""`thrust_arcs` for solutions of the 14-row variable-mass system (`lto_indirect_events_mass_batch`, DESIGN 4.19): `XC_all`
[14 x n_nodes x n_batch], `params` with Isp in the mass slot.  Per trajectory the named tuple of `thrust_arcs` plus propellant_kg
(read off the integrated mass), mass_final_kg = XC_all[7, 1, b] - propellant_kg and dv_rocket_ms = Isp 9.81 ln(m0 / mass_final)."""
function thrust_arcs_mass(ctx::LtoContext, XC_all::Array{Float64,3}, t_TU::Matrix{Float64}, params::Vector; max_events::Integer = 64,
                          integ::LtoIntegrator = LtoIntegrator())
    ndim, n_nodes, B = size(XC_all)
    ndim == 14 || throw(ArgumentError("XC_all must be [14 x n_nodes x n_batch]"))
    prm = [LtoParams(q) for q in params]
    n_events = zeros(Cint, B); t_event = fill(NaN, max_events, B); kind = zeros(Cint, max_events, B); on0 = zeros(Cint, B)
    dv = zeros(B); burn = zeros(B); prop = zeros(B); status = zeros(Cint, B)
    rc = ccall((:lto_indirect_events_mass_batch, liblto), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{LtoParams}, Cint, Ref{LtoIntegrator}, Cint,
                Ptr{Cint}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                Ptr{Cint}),
               ctx.handle, n_nodes, B, XC_all, t_TU, B, prm, length(prm), Ref(integ), max_events, n_events, t_event, kind, on0,
               dv, burn, C_NULL, prop, C_NULL, status)
    check(ctx, rc)
    map(1:B) do b
        arcs = Tuple{Float64,Float64}[]
        on = on0[b] != 0; mark = t_TU[1, b]
        for k in 1:min(n_events[b], max_events)
            isnan(t_event[k, b]) && break
            on ? push!(arcs, (mark, t_event[k, b])) : (mark = t_event[k, b])
            on = !on
        end
        (on && status[b] == 0) && push!(arcs, (mark, t_TU[end, b]))
        m0 = XC_all[7, 1, b]; mf = m0 - prop[b]
        isp = prm[length(prm) == 1 ? 1 : b].mass
        (arcs = arcs, dv = dv[b], burn_time = burn[b], n_events = Int(n_events[b]), status = Int(status[b]),
         propellant_kg = prop[b], mass_final_kg = mf, dv_rocket_ms = isp * 9.81 * log(m0 / mf))
    end
end

"""Control replay (`lto_control_replay_batch`, DESIGN 4.22): fly the history `lamv` [3 x n_knots x n_hist] of lambda_v, given at
the knots LinRange(t0, t1, n_knots) with n_hist = 1 or n_batch, from the starts `x0` [nstate x n_batch] (nstate 6: r, v with the
constant `mass` of the parameters; nstate 7: r, v, m with Isp in the mass slot).  The control is the natural cubic spline of `lamv`,
integrated knot interval by knot interval.  Returns the named tuple (x_final [nstate x B], dv [B] in DU/TU, accepted, rejected,
status [B], samples [nstate x n_samples x B] at the knots k with k % sample_every == 0 and the last one; `nothing` for
sample_every = 0)."""
function control_replay(ctx::LtoContext, x0::Matrix{Float64}, lamv::Array{Float64,3}, t0::Real, t1::Real, params::Vector;
                        sample_every::Integer = 0, integ::LtoIntegrator = LtoIntegrator())
    nstate, B = size(x0)
    size(lamv, 1) == 3 || throw(ArgumentError("lamv must be [3 x n_knots x n_hist]"))
    n_knots, n_hist = size(lamv, 2), size(lamv, 3)
    prm = [LtoParams(q) for q in params]
    last = n_knots - 1
    ns = sample_every > 0 ? div(last, sample_every) + 1 + (last % sample_every != 0 ? 1 : 0) : 0
    x_final = zeros(nstate, B); samples = zeros(nstate, max(ns, 1), B); dv = zeros(B)
    accepted = zeros(Cint, B); rejected = zeros(Cint, B); status = zeros(Cint, B)
    rc = ccall((:lto_control_replay_batch, liblto), Cint,
               (Ptr{Cvoid}, Cint, Cint, Cint, Cdouble, Cdouble, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{LtoParams}, Cint,
                Ref{LtoIntegrator}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}),
               ctx.handle, nstate, n_knots, B, Float64(t0), Float64(t1), lamv, n_hist, x0, prm, length(prm), Ref(integ), sample_every,
               x_final, samples, dv, accepted, rejected, status)
    check(ctx, rc)
    (x_final = x_final, dv = dv, accepted = Int.(accepted), rejected = Int.(rejected), status = Int.(status),
     samples = ns > 0 ? samples : nothing)
end

"""Neighbouring-extremal feedback gains (`lto_guidance_gains_batch`, DESIGN 4.23) of the 12-row solutions `XC` [12 x n x B] on the
grids `t` [n x n_tgrids] (n_tgrids = 1 or B): the segment STMs are swept on the device and turned into gains by the backward
recurrence that keeps the linearised arrival state fixed.  Returns the named tuple (K [6 x 6 x (n-1) x B] with
d lambda_k = K[:, :, k, b] d x_k, pivot [(n-1) x B], status [B]: 0 ok, 2 not finite, 3 a pivot ratio below sing_tol -- K is NaN from
that node down to node 0)."""
function guidance_gains(ctx::LtoContext, XC::Array{Float64,3}, t::Matrix{Float64}, params::Vector;
                        sing_tol::Real = 1e-10, integ::LtoIntegrator = LtoIntegrator())
    ndim, n, B = size(XC)
    prm = [LtoParams(q) for q in params]
    K = zeros(6, 6, n - 1, B); pivot = zeros(n - 1, B); status = zeros(Cint, B)
    rc = ccall((:lto_guidance_gains_batch, liblto), Cint,
               (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{LtoParams}, Cint, Ref{LtoIntegrator}, Cdouble,
                Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
               ctx.handle, ndim, n, B, XC, t, size(t, 2), prm, length(prm), Ref(integ), Float64(sing_tol), K, pivot, status)
    check(ctx, rc)
    (K = K, pivot = pivot, status = Int.(status))
end

"""Guided flight (`lto_guided_flight_batch`, DESIGN 4.23): the starts `x0` [6 x B] flown about the nominal `XC_nom` [12 x n x n_nom]
with node times `t` [n x n_nom] and gains `K` [6 x 6 x (n-1) x n_nom] (n_nom = 1 or B).  At node k with k % update_every == 0 the
costate is reset to lambda_nom,k + K_k (x - x_nom,k + e_j), e_j = nav[:, j, b] (`nav` [6 x n_upd x B] or `nothing`);
update_every = 0 never updates.  Returns the named tuple (x_final, lam_final [6 x B], dv [B] in DU/TU, nodes [6 x n x B],
accepted, rejected, status [B])."""
function guided_flight(ctx::LtoContext, XC_nom::Array{Float64,3}, t::Matrix{Float64}, K::Array{Float64,4}, x0::Matrix{Float64},
                       params::Vector; update_every::Integer = 1, nav::Union{Nothing,Array{Float64,3}} = nothing,
                       integ::LtoIntegrator = LtoIntegrator())
    ndim, n, n_nom = size(XC_nom)
    B = size(x0, 2)
    prm = [LtoParams(q) for q in params]
    x_final = zeros(6, B); lam_final = zeros(6, B); dv = zeros(B); nodes = zeros(6, n, B)
    accepted = zeros(Cint, B); rejected = zeros(Cint, B); status = zeros(Cint, B)
    rc = ccall((:lto_guided_flight_batch, liblto), Cint,
               (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble},
                Ptr{LtoParams}, Cint, Ref{LtoIntegrator}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint},
                Ptr{Cint}, Ptr{Cint}),
               ctx.handle, ndim, n, B, XC_nom, t, K, n_nom, x0, update_every, nav === nothing ? C_NULL : nav, prm, length(prm),
               Ref(integ), x_final, lam_final, dv, nodes, accepted, rejected, status)
    check(ctx, rc)
    (x_final = x_final, lam_final = lam_final, dv = dv, nodes = nodes, accepted = Int.(accepted), rejected = Int.(rejected),
     status = Int.(status))
end

"""`guidance_gains` for solutions of the 14-row variable-mass system (`lto_guidance_gains_mass_batch`, DESIGN 4.24): `XC`
[14 x n x B], Isp in the mass slot of the parameters.  The gains keep d r_f = d v_f = 0 and d lambda_m(t_f) = 0; the final mass is
free.  Returns the named tuple (K [7 x 7 x (n-1) x B], pivot [(n-1) x B], status [B])."""
function guidance_gains_mass(ctx::LtoContext, XC::Array{Float64,3}, t::Matrix{Float64}, params::Vector;
                             sing_tol::Real = 1e-10, integ::LtoIntegrator = LtoIntegrator())
    ndim, n, B = size(XC)
    ndim == 14 || throw(ArgumentError("XC must be [14 x n x B]"))
    prm = [LtoParams(q) for q in params]
    K = zeros(7, 7, n - 1, B); pivot = zeros(n - 1, B); status = zeros(Cint, B)
    rc = ccall((:lto_guidance_gains_mass_batch, liblto), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{LtoParams}, Cint, Ref{LtoIntegrator}, Cdouble,
                Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
               ctx.handle, n, B, XC, t, size(t, 2), prm, length(prm), Ref(integ), Float64(sing_tol), K, pivot, status)
    check(ctx, rc)
    (K = K, pivot = pivot, status = Int.(status))
end

"""`guided_flight` for the 14-row variable-mass system (`lto_guided_flight_mass_batch`, DESIGN 4.24): the starts `x0` [7 x B]
(r, v, m) flown about the nominal `XC_nom` [14 x n x n_nom] with gains `K` [7 x 7 x (n-1) x n_nom]; `nav` [7 x n_upd x B] or
`nothing`.  The update resets all seven costates from the seven measured states.  Returns the named tuple (x_final, lam_final
[7 x B] -- x_final[7, b] the final mass --, dv [B], nodes [7 x n x B], accepted, rejected, status [B])."""
function guided_flight_mass(ctx::LtoContext, XC_nom::Array{Float64,3}, t::Matrix{Float64}, K::Array{Float64,4},
                            x0::Matrix{Float64}, params::Vector; update_every::Integer = 1,
                            nav::Union{Nothing,Array{Float64,3}} = nothing, integ::LtoIntegrator = LtoIntegrator())
    ndim, n, n_nom = size(XC_nom)
    ndim == 14 || throw(ArgumentError("XC_nom must be [14 x n x n_nom]"))
    B = size(x0, 2)
    prm = [LtoParams(q) for q in params]
    x_final = zeros(7, B); lam_final = zeros(7, B); dv = zeros(B); nodes = zeros(7, n, B)
    accepted = zeros(Cint, B); rejected = zeros(Cint, B); status = zeros(Cint, B)
    rc = ccall((:lto_guided_flight_mass_batch, liblto), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble},
                Ptr{LtoParams}, Cint, Ref{LtoIntegrator}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint},
                Ptr{Cint}, Ptr{Cint}),
               ctx.handle, n, B, XC_nom, t, K, n_nom, x0, update_every, nav === nothing ? C_NULL : nav, prm, length(prm),
               Ref(integ), x_final, lam_final, dv, nodes, accepted, rejected, status)
    check(ctx, rc)
    (x_final = x_final, lam_final = lam_final, dv = dv, nodes = nodes, accepted = Int.(accepted), rejected = Int.(rejected),
     status = Int.(status))
end

"""Linear covariance of the guided flight (`lto_guidance_covariance_batch`, DESIGN 4.31) about the solutions `XC` [ndim x n x B],
ndim 12 or 14 (NX = ndim / 2; 14 rows: Isp in the mass slot of the parameters), on the grids `t` [n x n_tgrids].  The cases
`P0`, `R` [NX x NX x n_cases] and `update_every` [n_cases] (each >= 0) are shared by all trajectories: one call sweeps the STMs,
builds the gains and runs the forward pass of every (trajectory, case).  Returns the named tuple (P_final [NX x NX x n_cases x B],
P_nodes [NX x NX x n x n_cases x B] or `nothing`, cov_status [n_cases x B]: 0 ok, 2 not finite; K, pivot, gain_status as
`guidance_gains`; Phi [ndim x ndim x (n-1) x B] or `nothing`)."""
function guidance_covariance(ctx::LtoContext, XC::Array{Float64,3}, t::Matrix{Float64}, params::Vector, P0::Array{Float64,3},
                             R::Array{Float64,3}, update_every::Vector{<:Integer}; sing_tol::Real = 1e-10,
                             integ::LtoIntegrator = LtoIntegrator(), with_nodes::Bool = false, with_phi::Bool = false)
    ndim, n, B = size(XC)
    (ndim == 12 || ndim == 14) || throw(ArgumentError("XC must be [12 x n x B] or [14 x n x B]"))
    nx = ndim ÷ 2
    nc = length(update_every)
    (nc >= 1 && size(P0) == (nx, nx, nc) && size(R) == (nx, nx, nc)) ||
        throw(ArgumentError("P0 and R must be [NX x NX x n_cases] with one update_every per case"))
    all(>=(0), update_every) || throw(ArgumentError("update_every must be >= 0"))
    prm = [LtoParams(q) for q in params]
    every = Cint.(update_every)
    K = zeros(nx, nx, n - 1, B); pivot = zeros(n - 1, B); gain_status = zeros(Cint, B)
    Phi = with_phi ? zeros(ndim, ndim, n - 1, B) : nothing
    P_nodes = with_nodes ? zeros(nx, nx, n, nc, B) : nothing
    P_final = zeros(nx, nx, nc, B); cov_status = zeros(Cint, nc, B)
    rc = ccall((:lto_guidance_covariance_batch, liblto), Cint,
               (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{LtoParams}, Cint, Ref{LtoIntegrator}, Cdouble,
                Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble},
                Ptr{Cdouble}, Ptr{Cint}),
               ctx.handle, ndim, n, B, XC, t, size(t, 2), prm, length(prm), Ref(integ), Float64(sing_tol), nc, P0, R, every, K, pivot,
               gain_status, Phi === nothing ? C_NULL : Phi, P_nodes === nothing ? C_NULL : P_nodes, P_final, cov_status)
    check(ctx, rc)
    (P_final = P_final, P_nodes = P_nodes, cov_status = Int.(cov_status), K = K, pivot = pivot, gain_status = Int.(gain_status),
     Phi = Phi)
end

# ---------------------------------------------------------------------------------------------- direct
"defectCalc of multiShoot_CRTBP_direct: returns (defect1[nstate x (n_nodes-1)], errors[n_nodes-1])."
function direct_defectCalc(ctx::LtoHandle, X_all::Matrix{Float64}, u_all::Matrix{Float64}, t_TU::Vector{Float64},
                           nstate, n_nodes, nsteps, Isp, MU, DU, TU)
    defect1 = zeros(nstate, n_nodes - 1)
    errors = zeros(n_nodes - 1)
    prm = Ref(LtoDirectParams(MU, DU, TU, Isp))
    rc = ccall(entry(ctx, :direct_defect), Cint,
               (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Ref{LtoDirectParams},
                Ptr{Cdouble}, Ptr{Cdouble}),
               ctx.handle, nstate, n_nodes, 1, X_all, u_all, t_TU, 1, nsteps, prm, defect1, errors)
    check(ctx, rc)
    (defect1, errors)
end

"""Mid-point propagation of meshRefine_direct (direct.jl:645-656) for every segment in one sweep: returns
(x_mid[nstate x (n_nodes-1)], defect1, errors).  `nsteps = 2` reproduces the reference's single `ode7` step."""
function direct_midpoints(ctx::LtoContext, X_all::Matrix{Float64}, u_all::Matrix{Float64}, t_TU::Vector{Float64},
                          nstate, n_nodes, nsteps, Isp, MU, DU, TU)
    x_mid = zeros(nstate, n_nodes - 1)
    defect1 = zeros(nstate, n_nodes - 1)
    errors = zeros(n_nodes - 1)
    prm = Ref(LtoDirectParams(MU, DU, TU, Isp))
    rc = ccall((:lto_direct_midpoints, liblto), Cint,
               (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Ref{LtoDirectParams},
                Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
               ctx.handle, nstate, n_nodes, 1, X_all, u_all, t_TU, 1, nsteps, prm, x_mid, defect1, errors)
    check(ctx, rc)
    (x_mid, defect1, errors)
end

"""meshRefine_direct (direct.jl:597-680) in one library call with the trajectory resident on the GPU (`lto_direct_refine`,
DESIGN 4.14): nodes are removed while the smallest RKF7(8) estimate is below `tol_min`, then segments are bisected while the
largest is above `tol_max` and the mesh has fewer than `max_nodes` nodes.  Returns (X_all, u_all, t_TU, n_nodes) as the
reference does, then (n_removed, passes, status, errors): status 0 refined, 1 stopped at `max_nodes`, 2 a NaN estimate."""
function direct_refine(ctx::LtoContext, X_all::Matrix{Float64}, u_all::Matrix{Float64}, t_TU::Vector{Float64},
                       nstate, n_nodes, nsteps, Isp, MU, DU, TU; tol_min = 1e-20, tol_max = 1e-18, max_nodes = 4 * n_nodes)
    X_out = zeros(nstate, max_nodes)
    U_out = zeros(3, max_nodes)
    t_out = zeros(max_nodes)
    errors = zeros(max_nodes - 1)
    n_out = Ref{Cint}(0)
    n_removed = Ref{Cint}(0)
    passes = Ref{Cint}(0)
    status = Ref{Cint}(0)
    prm = Ref(LtoDirectParams(MU, DU, TU, Isp))
    rc = ccall((:lto_direct_refine, liblto), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ref{LtoDirectParams}, Cdouble, Cdouble, Cint,
                Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Cint}, Ref{Cint}, Ref{Cint}, Ref{Cint}, Ptr{Cdouble}),
               ctx.handle, nstate, n_nodes, X_all, u_all, t_TU, nsteps, prm, tol_min, tol_max, max_nodes, X_out, U_out, t_out,
               n_out, n_removed, passes, status, errors)
    check(ctx, rc)
    n = Int(n_out[])
    (X_out[:, 1:n], U_out[:, 1:n], t_out[1:n], n, Int(n_removed[]), Int(passes[]), Int(status[]), errors[1:n-1])
end

"""Direct solutions resampled onto one node count `n_new` in one library call (`lto_direct_resample_batch`, DESIGN 4.17): the new
grid equidistributes the RKF7(8) estimates (weight e^(1/8), floored at `w_floor` times the largest; `weights` replace them, with
`passes = 1`), the new nodes lie on the transcription's own half-arcs.  X [nstate x n_cap x n_batch], U [3 x n_cap x n_batch],
t [n_cap x n_batch]; `n_in` = the valid columns of every trajectory, as `lto_direct_refine_batch` leaves them (nothing: all).
Returns (X, U, t, errors_before, errors_after, status): status 0, 1 the new times were not strictly increasing, 2 a NaN estimate
(the outputs of such a trajectory are NaN)."""
function direct_resample(ctx::LtoContext, X::Array{Float64,3}, U::Array{Float64,3}, t::Matrix{Float64}, nsteps, Isp, MU, DU, TU,
                         n_new; n_in::Union{Nothing,Vector{Cint}} = nothing, weights::Union{Nothing,Matrix{Float64}} = nothing,
                         w_floor = 0.1, passes = 1)
    nstate, n_cap, n_batch = size(X)
    X_out = zeros(nstate, n_new, n_batch)
    U_out = zeros(3, n_new, n_batch)
    t_out = zeros(n_new, n_batch)
    errors_before = zeros(n_cap - 1, n_batch)
    errors_after = zeros(n_new - 1, n_batch)
    status = zeros(Cint, n_batch)
    prm = Ref(LtoDirectParams(MU, DU, TU, Isp))
    rc = ccall((:lto_direct_resample_batch, liblto), Cint,
               (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Cint, Ref{LtoDirectParams}, Cint,
                Ptr{Cdouble}, Cdouble, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
               ctx.handle, nstate, n_cap, n_batch, X, U, t, n_in === nothing ? C_NULL : n_in, nsteps, prm, n_new,
               weights === nothing ? C_NULL : weights, w_floor, passes, X_out, U_out, t_out, errors_before, errors_after, status)
    check(ctx, rc)
    (X_out, U_out, t_out, errors_before, errors_after, Int.(status))
end

"""jacobianCalc + tf partial of multiShoot_CRTBP_direct: Jac_full [nstate(n_nodes-1) x n_nodes(nstate+3)+1]
(state columns node-major, then control columns, then tf: direct.jl:146-162, :516).  The blocks come from the
variational equations integrated on the GPU, not from 18 perturbed re-propagations per segment."""
function direct_jacobianCalc(ctx::LtoHandle, X_all::Matrix{Float64}, u_all::Matrix{Float64}, t_TU::Vector{Float64},
                             nstate, n_nodes, nsteps, Isp, MU, DU, TU)
    nvar = 2 * (nstate + 3)
    S = n_nodes - 1
    Jac_temp = zeros(nstate, nvar, S)
    ddefect_dt = zeros(nstate, S)
    defect1 = zeros(nstate, S)
    errors = zeros(S)
    prm = Ref(LtoDirectParams(MU, DU, TU, Isp))
    rc = ccall(entry(ctx, :direct_jacobian), Cint,
               (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Ref{LtoDirectParams},
                Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
               ctx.handle, nstate, n_nodes, 1, X_all, u_all, t_TU, 1, nsteps, prm, Jac_temp, ddefect_dt, defect1, errors)
    check(ctx, rc)
    Jac_full = zeros(nstate * S, n_nodes * (nstate + 3) + 1)
    for i = 1:S
        rows = (i - 1) * nstate + 1 : i * nstate
        Jac_full[rows, (i - 1) * nstate + 1 : (i + 1) * nstate] = Jac_temp[:, 1:2 * nstate, i]
        Jac_full[rows, nstate * n_nodes + 3 * (i - 1) + 1 : nstate * n_nodes + 3 * (i - 1) + 6] = Jac_temp[:, 2 * nstate + 1 : end, i]
    end
    Jac_full[:, end] = ddefect_dt[:]
    (Jac_full, defect1, errors)
end

# ------------------------------------------------------------------------------------------- device-resident API
# optimizeTraj of multiShoot_CRTBP_direct (direct.jl:248-403) for flagEnd = false: one Jacobian sweep and the exact QP step on the
# device.  state_0 / state_f from interpEndStates.  Returns (x_update, u_update, dV1_update, dV2_update, cost).
function direct_qp_step(ctx::LtoContext, X_all::Matrix{Float64}, u_all::Matrix{Float64}, t_TU::Vector{Float64}, nsteps, Isp,
                        MU, DU, TU, state_0, state_f, mass, dV1, dV2; allowImpulsive::Bool = false)
    nstate, n_nodes = size(X_all)
    dX = zeros(nstate, n_nodes); dU = zeros(3, n_nodes); dV = zeros(6); cost = zeros(1)
    prm = Ref(LtoDirectParams(MU, DU, TU, Isp))
    tg = Ref(LtoDirectTargets(state_0, state_f, mass, dV1, dV2))
    rc = ccall(entry(ctx, :direct_qp_step), Cint,
               (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Ref{LtoDirectParams},
                Ref{LtoDirectTargets}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
               ctx.handle, nstate, n_nodes, 1, X_all, u_all, t_TU, 1, nsteps, prm, tg, 1, allowImpulsive, dX, dU, dV, cost)
    check(ctx, rc)
    (dX, dU, dV[1:3], dV[4:6], cost[1])
end

# Costates of a direct solution from the multipliers of a frozen QP step at the given point (lto_direct_costates; covector mapping):
# returns (Lambda [nstate x n], mult [nstate x (n-1)], XC [12 x n] = (X; c^2 Lambda) with c = TU^2 / DU / 1e3 / 1000 -- the node
# vector of the indirect method for p = 2, `nothing` for nstate = 7 --, kkt_res, status).
function direct_costates(ctx::LtoContext, X_all::Matrix{Float64}, u_all::Matrix{Float64}, t_TU::Vector{Float64}, nsteps, Isp,
                         MU, DU, TU, state_0, state_f, mass, dV1, dV2; allowImpulsive::Bool = false)
    nstate, n_nodes = size(X_all)
    Lambda = zeros(nstate, n_nodes); mult = zeros(nstate, n_nodes - 1); res = zeros(1); status = zeros(Cint, 1)
    XC = nstate == 6 ? zeros(12, n_nodes) : nothing
    prm = Ref(LtoDirectParams(MU, DU, TU, Isp))
    tg = Ref(LtoDirectTargets(state_0, state_f, mass, dV1, dV2))
    rc = ccall(entry(ctx, :direct_costates), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ref{LtoDirectParams}, Ref{LtoDirectTargets},
                Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
               ctx.handle, nstate, n_nodes, X_all, u_all, t_TU, nsteps, prm, tg, allowImpulsive, Lambda, mult,
               XC === nothing ? Ptr{Cdouble}(C_NULL) : pointer(XC), res, status)
    check(ctx, rc)
    (Lambda, mult, XC, res[1], Int(status[1]))
end

# The loop of multiShoot_CRTBP_direct (direct.jl:477-594) on the device: returns (X_all, u_all, t_TU, dV1, dV2, defect,
# status, iterations, history [3 x maxIter] = (max|defect|, cost, alpha)); status 0 converged, 1 maxIter, 2 NaN, 3 singular.
function direct_solve(ctx::LtoContext, X_all::Matrix{Float64}, u_all::Matrix{Float64}, t_TU::Vector{Float64}, nsteps, Isp,
                      MU, DU, TU, state_0, state_f, mass, dV1, dV2, maxIter::Integer; allowImpulsive::Bool = false)
    nstate, n_nodes = size(X_all)
    Xo = zeros(nstate, n_nodes); Uo = zeros(3, n_nodes); dV = zeros(6); to = zeros(n_nodes); defect = zeros(nstate, n_nodes - 1)
    status = zeros(Cint, 1); iters = zeros(Cint, 1); hist = fill(NaN, 3, max(maxIter, 1))
    prm = Ref(LtoDirectParams(MU, DU, TU, Isp))
    tg = Ref(LtoDirectTargets(state_0, state_f, mass, dV1, dV2))
    rc = ccall(entry(ctx, :direct_solve), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ref{LtoDirectParams}, Ref{LtoDirectTargets},
                Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}),
               ctx.handle, nstate, n_nodes, X_all, u_all, t_TU, nsteps, prm, tg, allowImpulsive, maxIter, Xo, Uo, dV, to, defect,
               status, iters, hist)
    check(ctx, rc)
    (Xo, Uo, to, dV[1:3], dV[4:6], defect, Int(status[1]), Int(iters[1]), hist[:, 1:maxIter])
end

# Free end points (flagEnd = true, direct.jl:278-292, :353-369, :521-569).  X0_states / Xf_states are [6 x n] (rows = state).
_orbits(X0_times, X0_states, Xf_times, Xf_states) =
    LtoDirectOrbits(length(X0_times), length(Xf_times), pointer(X0_times), pointer(X0_states), pointer(Xf_times), pointer(Xf_states))

# End targets and end model at (tau1, tau2) on the device: returns (state_0, state_f, LtoDirectEndModel).
function direct_end_states(ctx::LtoContext, τ1, τ2, X0_times::Vector{Float64}, X0_states::Matrix{Float64}, Xf_times::Vector{Float64},
                           Xf_states::Matrix{Float64})
    tau = [Float64(τ1), Float64(τ2)]; s = zeros(12); model = Ref(LtoDirectEndModel(zeros(6), zeros(6), 0.0, 0.0))
    rc = GC.@preserve X0_times X0_states Xf_times Xf_states begin
        ob = Ref(_orbits(X0_times, X0_states, Xf_times, Xf_states))
        ccall(entry(ctx, :direct_end_states), Cint,
              (Ptr{Cvoid}, Ref{LtoDirectOrbits}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ref{LtoDirectEndModel}), ctx.handle, ob, 1, tau, s, model)
    end
    check(ctx, rc)
    (s[1:6], s[7:12], model[])
end

# The trajectory-stacking initial guess of the reference demos (CRTBP_Multishoot_direct_demo.jl:116-157) for B starts side by side
# (`lto_stack_guess_batch`, DESIGN 4.15): per start tof1 TU ballistically on the departure orbit from phase tau1, the closest point
# of the arrival orbit (find_tau), tof2 TU ballistically from there, n_nodes samples over LinRange(0, tof1 + tof2, n_nodes), the last
# one snapped onto the arrival orbit.  Returns (X [6 x n_nodes x B], t [n_nodes x B], tau [3 x B] = (tau1 wrapped; tau2 at the
# junction; tau2 at the end), gap [2 x B], status [B]).
function stack_guess(ctx::LtoContext, tau1::Vector{Float64}, tof1::Vector{Float64}, tof2::Vector{Float64}, n_nodes::Integer,
                     X0_times::Vector{Float64}, X0_states::Matrix{Float64}, Xf_times::Vector{Float64}, Xf_states::Matrix{Float64},
                     MU; integ::LtoIntegrator = LtoIntegrator())
    B = length(tau1)
    (length(tof1) == B && length(tof2) == B) || error("stack_guess: tau1, tof1 and tof2 need one entry per start")
    X = zeros(6, n_nodes, B); t = zeros(n_nodes, B); tau = zeros(3, B); gap = zeros(2, B); status = zeros(Cint, B)
    rc = GC.@preserve X0_times X0_states Xf_times Xf_states begin
        ob = Ref(_orbits(X0_times, X0_states, Xf_times, Xf_states))
        ccall((:lto_stack_guess_batch, liblto), Cint,
              (Ptr{Cvoid}, Cint, Cint, Cdouble, Ref{LtoDirectOrbits}, Ref{LtoIntegrator}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
               Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
              ctx.handle, n_nodes, B, Float64(MU), ob, Ref(integ), tau1, tof1, tof2, X, t, tau, gap, status)
    end
    check(ctx, rc)
    (X, t, tau, gap, Int.(status))
end

# The differential corrector of periodic orbits with the xz-plane symmetry (`lto_halo_correct_batch`, DESIGN 4.25) for B seeds side by
# side: seeds [6 x B] = (x0, ., z0, ., vy0, .), mode 0 hold z0 / 1 hold x0 / 2 planar.  Returns (state [6 x B], period [B], resid [B],
# iterations [B], history [(max_iter + 1) x B], status [B]).
function halo_correct(ctx::LtoContext, seeds::Matrix{Float64}, mode::Integer, MU; tol = 1e-12, max_iter::Integer = 15, t_max = 10.0,
                      sing_tol = 1e-12, integ::LtoIntegrator = LtoIntegrator())
    size(seeds, 1) == 6 || error("halo_correct: seeds must be 6 x B")
    B = size(seeds, 2)
    state = zeros(6, B); period = zeros(B); resid = zeros(B); hist = zeros(max_iter + 1, B)
    its = zeros(Cint, B); status = zeros(Cint, B)
    rc = ccall((:lto_halo_correct_batch, liblto), Cint,
               (Ptr{Cvoid}, Cint, Cdouble, Cint, Ptr{Cdouble}, Cdouble, Cint, Cdouble, Cdouble, Ref{LtoIntegrator}, Ptr{Cdouble},
                Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cint}),
               ctx.handle, B, Float64(MU), mode, seeds, Float64(tol), max_iter, Float64(t_max), Float64(sing_tol), Ref(integ), state,
               period, resid, its, hist, status)
    check(ctx, rc)
    (state, period, resid, Int.(its), hist, Int.(status))
end

# Periodic orbits at a given Jacobi constant (what = 0) or period (what = 1) (`lto_halo_target_batch`, DESIGN 4.27): seeds [6 x B],
# targets [K x B] -- orbit b's K members are corrected one after another in one launch, each from the secant through the last two.
# Returns (state [6 x K x B], period, jacobi, resid, iterations [K x B], history [(max_iter + 1) x K x B], status [K x B]).
function halo_target(ctx::LtoContext, seeds::Matrix{Float64}, targets::Matrix{Float64}, what::Integer, MU; planar::Bool = false,
                     tol = 1e-12, max_iter::Integer = 15, t_max = 10.0, sing_tol = 1e-12, integ::LtoIntegrator = LtoIntegrator())
    size(seeds, 1) == 6 || error("halo_target: seeds must be 6 x B")
    B = size(seeds, 2)
    size(targets, 2) == B || error("halo_target: targets must be K x B")
    (what == 0 || what == 1) || error("halo_target: what must be 0 (Jacobi constant) or 1 (period)")
    K = size(targets, 1)
    state = zeros(6, K, B); period = zeros(K, B); jac = zeros(K, B); resid = zeros(K, B); hist = zeros(max_iter + 1, K, B)
    its = zeros(Cint, K, B); status = zeros(Cint, K, B)
    rc = ccall((:lto_halo_target_batch, liblto), Cint,
               (Ptr{Cvoid}, Cint, Cint, Cdouble, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Cint, Cdouble, Cdouble,
                Ref{LtoIntegrator}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cint}),
               ctx.handle, K, B, Float64(MU), planar ? 1 : 0, what, seeds, targets, Float64(tol), max_iter, Float64(t_max),
               Float64(sing_tol), Ref(integ), state, period, jac, resid, its, hist, status)
    check(ctx, rc)
    (state, period, jac, resid, Int.(its), hist, Int.(status))
end

# Families of periodic orbits by pseudo-arclength continuation (`lto_halo_arclength_batch`, DESIGN 4.28): seeds [6 x B], dir0 [3 x B]
# and ds0 [B]; orbit b's K members, their step halvings and the growth of ds run in one launch.  dir_is_tangent = false: member 0 is
# the seed corrected onto the family, the march leaves towards dir0; true: the seed is a point of the family and dir0 its tangent.
# Returns (state [6 x K x B], tangent [3 x K x B], det, ds [K x B], halvings, period, jacobi, resid, iterations [K x B],
# history [(max_iter + 1) x K x B], status [K x B]).
function halo_arclength(ctx::LtoContext, seeds::Matrix{Float64}, dir0::Matrix{Float64}, ds0::Vector{Float64}, n_members::Integer, MU;
                        planar::Bool = false, dir_is_tangent::Bool = false, ds_min = minimum(ds0) / 1024, ds_max = maximum(ds0),
                        grow = 1.0, fast_iter::Integer = 3, cos_min = 0.0, tol = 1e-12, max_iter::Integer = 15, t_max = 10.0,
                        sing_tol = 1e-12, integ::LtoIntegrator = LtoIntegrator())
    size(seeds, 1) == 6 || error("halo_arclength: seeds must be 6 x B")
    B = size(seeds, 2)
    size(dir0) == (3, B) || error("halo_arclength: dir0 must be 3 x B")
    length(ds0) == B || error("halo_arclength: one ds0 per orbit")
    K = Int(n_members)
    state = zeros(6, K, B); tangent = zeros(3, K, B); det = zeros(K, B); ds = zeros(K, B); period = zeros(K, B); jac = zeros(K, B)
    resid = zeros(K, B); hist = zeros(max_iter + 1, K, B)
    halv = zeros(Cint, K, B); its = zeros(Cint, K, B); status = zeros(Cint, K, B)
    rc = ccall((:lto_halo_arclength_batch, liblto), Cint,
               (Ptr{Cvoid}, Cint, Cint, Cdouble, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Cdouble, Cdouble, Cint,
                Cdouble, Cdouble, Cint, Cdouble, Cdouble, Ref{LtoIntegrator}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cint}),
               ctx.handle, K, B, Float64(MU), planar ? 1 : 0, dir_is_tangent ? 1 : 0, seeds, dir0, ds0, Float64(ds_min), Float64(ds_max),
               Float64(grow), fast_iter, Float64(cos_min), Float64(tol), max_iter, Float64(t_max), Float64(sing_tol), Ref(integ),
               state, tangent, det, ds, halv, period, jac, resid, its, hist, status)
    check(ctx, rc)
    (state, tangent, det, ds, Int.(halv), period, jac, resid, Int.(its), hist, Int.(status))
end

# One revolution of B periodic orbits from (state0 [6 x B], period [B]) at n_samples equal times, the state-transition matrix carried
# through (`lto_halo_table_batch`, DESIGN 4.25).  Returns (times [n], X [6 x n x B], M [6 x 6 x B], closure [B], jacobi [2 x B],
# nu [2 x B], status [B]); (times, X[:, :, b]) is an orbit table as interpEndStates and direct_solve_free take it.
function halo_table(ctx::LtoContext, state0::Matrix{Float64}, period::Vector{Float64}, n_samples::Integer, MU;
                    integ::LtoIntegrator = LtoIntegrator())
    size(state0, 1) == 6 || error("halo_table: state0 must be 6 x B")
    B = size(state0, 2)
    length(period) == B || error("halo_table: one period per orbit")
    X = zeros(6, n_samples, B); times = zeros(n_samples); M = zeros(6, 6, B); closure = zeros(B); jac = zeros(2, B); nu = zeros(2, B)
    status = zeros(Cint, B)
    rc = ccall((:lto_halo_table_batch, liblto), Cint,
               (Ptr{Cvoid}, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ref{LtoIntegrator}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
               ctx.handle, n_samples, B, Float64(MU), state0, period, Ref(integ), X, times, M, closure, jac, nu, status)
    check(ctx, rc)
    (times, X, M, closure, jac, nu, Int.(status))
end

# The eigen-directions of B periodic orbits at the phases tau and the perturbed starts (`lto_halo_manifold_seeds_batch`, DESIGN 4.26):
# state0 [6 x B], period [B], M [6 x 6 x B] as halo_table returns it, tau [P] shared by the batch, eps the offset.  Returns (lambda
# [2 x B] = (lambda_u, lambda_s), X [6 x 2 x P x B], V [6 x 2 x P x B], starts [6 x 4 x P x B] in the order (u+, u-, s+, s-), status [B]).
function manifold_seeds(ctx::LtoContext, state0::Matrix{Float64}, period::Vector{Float64}, M::Array{Float64,3}, tau::Vector{Float64}, MU;
                        eps = 1e-6, integ::LtoIntegrator = LtoIntegrator())
    size(state0, 1) == 6 || error("manifold_seeds: state0 must be 6 x B")
    B = size(state0, 2)
    length(period) == B || error("manifold_seeds: one period per orbit")
    size(M) == (6, 6, B) || error("manifold_seeds: M must be 6 x 6 x B")
    P = length(tau)
    P >= 1 || error("manifold_seeds: at least one phase")
    lambda = zeros(2, B); X = zeros(6, 2, P, B); V = zeros(6, 2, P, B); starts = zeros(6, 4, P, B); status = zeros(Cint, B)
    rc = ccall((:lto_halo_manifold_seeds_batch, liblto), Cint,
               (Ptr{Cvoid}, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Ref{LtoIntegrator},
                Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
               ctx.handle, P, B, Float64(MU), state0, period, M, tau, Float64(eps), Ref(integ), lambda, X, V, starts, status)
    check(ctx, rc)
    (lambda, X, V, starts, Int.(status))
end

# Ballistic arcs from y0 [6 x N] over the signed times t_max [N] to the section y[sec_axis] = sec_value (`lto_section_flight_batch`,
# DESIGN 4.26; sec_axis counts from 0 as in C).  Returns (x_end [6 x N], t_end [N], count [N], dC [N], X [6 x n_samples x N], status [N]).
function section_flight(ctx::LtoContext, y0::Matrix{Float64}, t_max::Vector{Float64}, MU; sec_axis::Integer = 1, sec_value = 0.0,
                        sec_dir::Integer = 0, n_cross::Integer = 1, r_min::Vector{Float64} = [0.0, 0.0], n_samples::Integer = 0,
                        integ::LtoIntegrator = LtoIntegrator())
    size(y0, 1) == 6 || error("section_flight: y0 must be 6 x N")
    N = size(y0, 2)
    length(t_max) == N || error("section_flight: one t_max per arc")
    length(r_min) == 2 || error("section_flight: r_min has two entries")
    x_end = zeros(6, N); t_end = zeros(N); dC = zeros(N); X = zeros(6, n_samples, N); count = zeros(Cint, N); status = zeros(Cint, N)
    rc = ccall((:lto_section_flight_batch, liblto), Cint,
               (Ptr{Cvoid}, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cdouble, Cint, Cint, Ptr{Cdouble}, Cint, Ref{LtoIntegrator},
                Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
               ctx.handle, N, Float64(MU), y0, t_max, sec_axis, Float64(sec_value), sec_dir, n_cross, r_min, n_samples, Ref(integ),
               x_end, t_end, count, dC, X, status)
    check(ctx, rc)
    (x_end, t_end, Int.(count), dC, X, Int.(status))
end

# For each column of A [6 x nA] the nearest column of Bs [6 x nB] in sqrt(|dr|^2 + (w |dv|)^2) (`lto_state_match_batch`, DESIGN 4.26).
# Returns (index [nA], 1-based, 0 where every distance is NaN; dist [nA]; dr [nA]; dv [nA]).
function state_match(ctx::LtoContext, A::Matrix{Float64}, Bs::Matrix{Float64}; w = 1.0)
    size(A, 1) == 6 && size(Bs, 1) == 6 || error("state_match: A and Bs must have 6 rows")
    nA = size(A, 2); nB = size(Bs, 2)
    index = zeros(Cint, nA); dist = zeros(nA); dr = zeros(nA); dv = zeros(nA)
    rc = ccall((:lto_state_match_batch, liblto), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
               ctx.handle, nA, nB, A, Bs, Float64(w), index, dist, dr, dv)
    check(ctx, rc)
    (Int.(index) .+ 1, dist, dr, dv)
end

# The Floquet-mode station-keeping gains from the directions V [6 x 2 x P x B] of manifold_seeds (`lto_stationkeep_gains_batch`,
# DESIGN 4.29).  Returns (W [6 x P x B], G [3 x 6 x P x B], alpha [P x B], status [P x B]).
function stationkeep_gains(ctx::LtoContext, V::Array{Float64,4}; sing_tol = 1e-8)
    size(V, 1) == 6 && size(V, 2) == 2 || error("stationkeep_gains: V must be 6 x 2 x P x B")
    P = size(V, 3); B = size(V, 4)
    W = zeros(6, P, B); G = zeros(3, 6, P, B); alpha = zeros(P, B); status = zeros(Cint, P, B)
    rc = ccall((:lto_stationkeep_gains_batch, liblto), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
               ctx.handle, P, B, V, Float64(sing_tol), W, G, alpha, status)
    check(ctx, rc)
    (W, G, alpha, Int.(status))
end

# B runs from x0 [6 x B] under the impulsive feedback G [3 x 6 x n_man x n_orb] about X_ref [6 x n_man x n_orb] with the spans dt
# [n_man x n_orb], n_orb = 1 or B, for n_rev revolutions (`lto_stationkeep_flight_batch`, DESIGN 4.29).  nav [6 x n_upd x B] and exe
# [4 x n_upd x B] or nothing.  Returns (x_final [6 x B], dv_total [B], n_burn [B], dev [2 x n_upd x B], dv_hist [n_upd x B], dev_final
# [2 x B], accepted [B], rejected [B], status [B], lost_at [B], counted from 0 as in C, -1: not lost).
function stationkeep_flight(ctx::LtoContext, X_ref::Array{Float64,3}, dt::Matrix{Float64}, G::Array{Float64,4}, x0::Matrix{Float64},
                            n_rev::Integer, MU; nav = nothing, exe = nothing, dv_min = 0.0, dv_max = 0.0, r_lost = 0.0,
                            integ::LtoIntegrator = LtoIntegrator())
    size(x0, 1) == 6 || error("stationkeep_flight: x0 must be 6 x B")
    B = size(x0, 2)
    size(X_ref, 1) == 6 || error("stationkeep_flight: X_ref must be 6 x n_man x n_orb")
    n_man = size(X_ref, 2); n_orb = size(X_ref, 3)
    n_orb == 1 || n_orb == B || error("stationkeep_flight: one orbit or one per run")
    size(dt) == (n_man, n_orb) || error("stationkeep_flight: dt must be n_man x n_orb")
    size(G) == (3, 6, n_man, n_orb) || error("stationkeep_flight: G must be 3 x 6 x n_man x n_orb")
    n_upd = n_rev * n_man
    nav === nothing || size(nav) == (6, n_upd, B) || error("stationkeep_flight: nav must be 6 x n_upd x B")
    exe === nothing || size(exe) == (4, n_upd, B) || error("stationkeep_flight: exe must be 4 x n_upd x B")
    x_final = zeros(6, B); dv_total = zeros(B); dev = zeros(2, n_upd, B); dv_hist = zeros(n_upd, B); dev_final = zeros(2, B)
    n_burn = zeros(Cint, B); acc = zeros(Cint, B); rej = zeros(Cint, B); status = zeros(Cint, B); lost_at = zeros(Cint, B)
    rc = ccall((:lto_stationkeep_flight_batch, liblto), Cint,
               (Ptr{Cvoid}, Cint, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble},
                Ptr{Cdouble}, Cdouble, Cdouble, Cdouble, Ref{LtoIntegrator}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble},
                Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}),
               ctx.handle, n_man, n_rev, B, Float64(MU), X_ref, dt, G, n_orb, x0, nav === nothing ? C_NULL : nav,
               exe === nothing ? C_NULL : exe, Float64(dv_min), Float64(dv_max), Float64(r_lost), Ref(integ), x_final, dv_total, n_burn,
               dev, dv_hist, dev_final, acc, rej, status, lost_at)
    check(ctx, rc)
    (x_final, dv_total, Int.(n_burn), dev, dv_hist, dev_final, Int.(acc), Int.(rej), Int.(status), Int.(lost_at))
end

# The state-transition matrices between phases of B periodic orbits (`lto_halo_stm_batch`, DESIGN 4.30): state0 [6 x B], period [B],
# tau [P] the phases shared by the batch, horizons [K] in periods, > 0 and strictly increasing.  Returns (X [6 x P x B] the orbit
# point at each phase, Phi [6 x 6 x K x P x B] = Phi(t_j + h_k P, t_j), X_tgt [6 x K x P x B], accepted [P x B], rejected [P x B],
# status [P x B]).
function halo_stm(ctx::LtoContext, state0::Matrix{Float64}, period::Vector{Float64}, tau::Vector{Float64}, horizons::Vector{Float64},
                  MU; integ::LtoIntegrator = LtoIntegrator())
    size(state0, 1) == 6 || error("halo_stm: state0 must be 6 x B")
    B = size(state0, 2)
    length(period) == B || error("halo_stm: one period per orbit")
    P = length(tau); K = length(horizons)
    P >= 1 && K >= 1 || error("halo_stm: at least one phase and one horizon")
    X = zeros(6, P, B); Phi = zeros(6, 6, K, P, B); Xt = zeros(6, K, P, B)
    acc = zeros(Cint, P, B); rej = zeros(Cint, P, B); status = zeros(Cint, P, B)
    rc = ccall((:lto_halo_stm_batch, liblto), Cint,
               (Ptr{Cvoid}, Cint, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{LtoIntegrator},
                Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}),
               ctx.handle, P, K, B, Float64(MU), state0, period, tau, horizons, Ref(integ), X, Phi, Xt, acc, rej, status)
    check(ctx, rc)
    (X, Phi, Xt, Int.(acc), Int.(rej), Int.(status))
end

# The target-point station-keeping gains from Phi [6 x 6 x K x n] of halo_stm (`lto_stationkeep_target_gains_batch`, DESIGN 4.30):
# dv = G dx minimises q |dv|^2 + sum_k r[k] |position deviation at target k|^2.  Returns (G [3 x 6 x n], pivot [n], status [n]).
function stationkeep_target_gains(ctx::LtoContext, Phi::Array{Float64,4}; q = 1e-2, r::Vector{Float64} = ones(size(Phi, 3)),
                                  sing_tol = 1e-12)
    size(Phi, 1) == 6 && size(Phi, 2) == 6 || error("stationkeep_target_gains: Phi must be 6 x 6 x K x n")
    K = size(Phi, 3); n = size(Phi, 4)
    length(r) == K || error("stationkeep_target_gains: one weight per target")
    G = zeros(3, 6, n); pivot = zeros(n); status = zeros(Cint, n)
    rc = ccall((:lto_stationkeep_target_gains_batch, liblto), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
               ctx.handle, K, n, Phi, Float64(q), r, Float64(sing_tol), G, pivot, status)
    check(ctx, rc)
    (G, pivot, Int.(status))
end

# optimizeTraj with flagEnd = true: one Jacobian sweep and the exact free-end QP step.  Returns (x_update, u_update, p1_update,
# p2_update, dV1_update, dV2_update, cost).
function direct_qp_step_free(ctx::LtoContext, X_all::Matrix{Float64}, u_all::Matrix{Float64}, t_TU::Vector{Float64}, nsteps, Isp,
                             MU, DU, TU, state_0, state_f, model::LtoDirectEndModel, β, mass, dV1, dV2; allowImpulsive::Bool = false)
    nstate, n_nodes = size(X_all)
    dX = zeros(nstate, n_nodes); dU = zeros(3, n_nodes); dV = zeros(6); p = zeros(2); cost = zeros(1)
    prm = Ref(LtoDirectParams(MU, DU, TU, Isp))
    tg = Ref(LtoDirectTargets(state_0, state_f, mass, dV1, dV2))
    rc = ccall(entry(ctx, :direct_qp_step_free), Cint,
               (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Ref{LtoDirectParams},
                Ref{LtoDirectTargets}, Ref{LtoDirectEndModel}, Ref{Cdouble}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                Ptr{Cdouble}, Ptr{Cdouble}),
               ctx.handle, nstate, n_nodes, 1, X_all, u_all, t_TU, 1, nsteps, prm, tg, Ref(model), Ref(Cdouble(β)), 1, allowImpulsive,
               dX, dU, dV, p, cost)
    check(ctx, rc)
    (dX, dU, p[1], p[2], dV[1:3], dV[4:6], cost[1])
end

# The loop of multiShoot_CRTBP_direct with flagEnd on the device: returns (X_all, u_all, τ1, τ2, t_TU, dV1, dV2, defect, status,
# iterations, history [5 x maxIter] = (max|defect|, cost, alpha, τ1, τ2)).
function direct_solve_free(ctx::LtoContext, X_all::Matrix{Float64}, u_all::Matrix{Float64}, τ1, τ2, t_TU::Vector{Float64}, nsteps,
                           Isp, MU, DU, TU, X0_times::Vector{Float64}, X0_states::Matrix{Float64}, Xf_times::Vector{Float64},
                           Xf_states::Matrix{Float64}, flagEnd::Bool, β, mass, dV1, dV2, maxIter::Integer; allowImpulsive::Bool = false)
    nstate, n_nodes = size(X_all)
    Xo = zeros(nstate, n_nodes); Uo = zeros(3, n_nodes); dV = zeros(6); to = zeros(n_nodes); defect = zeros(nstate, n_nodes - 1)
    tau = [Float64(τ1), Float64(τ2)]; tau_o = zeros(2)
    status = zeros(Cint, 1); iters = zeros(Cint, 1); hist = fill(NaN, 5, max(maxIter, 1))
    prm = Ref(LtoDirectParams(MU, DU, TU, Isp))
    tg = Ref(LtoDirectTargets(zeros(6), zeros(6), mass, dV1, dV2))
    rc = GC.@preserve X0_times X0_states Xf_times Xf_states begin
        ob = Ref(_orbits(X0_times, X0_states, Xf_times, Xf_states))
        ccall(entry(ctx, :direct_solve_free), Cint,
              (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ref{LtoDirectParams}, Ref{LtoDirectOrbits},
               Ref{LtoDirectTargets}, Ptr{Cdouble}, Cdouble, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
               Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}),
              ctx.handle, nstate, n_nodes, X_all, u_all, t_TU, nsteps, prm, ob, tg, tau, β, flagEnd, allowImpulsive, maxIter, Xo, Uo,
              dV, to, defect, tau_o, status, iters, hist)
    end
    check(ctx, rc)
    (Xo, Uo, tau_o[1], tau_o[2], to, dV[1:3], dV[4:6], defect, Int(status[1]), Int(iters[1]), hist[:, 1:maxIter])
end

# Free time of flight (direct.jl:286-295, :503-516, :567, :582): tf_jump bounded by `step` per free iteration and tf by [tf_min,
# tf_max] (TU; tf_min past t0).  A Julia twin of lto_direct_tf_bounds.
struct LtoDirectTfBounds
    step::Cdouble
    tf_min::Cdouble
    tf_max::Cdouble
end

# optimizeTraj with flagEnd = true and a free tf: one Jacobian sweep with the tf column and the exact free-end, free-tf QP step
# (tf = t_TU[end]).  Returns (x_update, u_update, p1_update, p2_update, tf_update, dV1_update, dV2_update, cost).
function direct_qp_step_free_tf(ctx::LtoContext, X_all::Matrix{Float64}, u_all::Matrix{Float64}, t_TU::Vector{Float64}, nsteps, Isp,
                                MU, DU, TU, state_0, state_f, model::LtoDirectEndModel, β, tfb::LtoDirectTfBounds, mass, dV1, dV2;
                                allowImpulsive::Bool = false)
    nstate, n_nodes = size(X_all)
    dX = zeros(nstate, n_nodes); dU = zeros(3, n_nodes); dV = zeros(6); p = zeros(3); cost = zeros(1)
    prm = Ref(LtoDirectParams(MU, DU, TU, Isp))
    tg = Ref(LtoDirectTargets(state_0, state_f, mass, dV1, dV2))
    rc = ccall(entry(ctx, :direct_qp_step_free_tf), Cint,
               (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Ref{LtoDirectParams},
                Ref{LtoDirectTargets}, Ref{LtoDirectEndModel}, Ref{Cdouble}, Ref{LtoDirectTfBounds}, Cint, Cint, Ptr{Cdouble},
                Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
               ctx.handle, nstate, n_nodes, 1, X_all, u_all, t_TU, 1, nsteps, prm, tg, Ref(model), Ref(Cdouble(β)), Ref(tfb), 1,
               allowImpulsive, dX, dU, dV, p, cost)
    check(ctx, rc)
    (dX, dU, p[1], p[2], p[3], dV[1:3], dV[4:6], cost[1])
end

# The loop of multiShoot_CRTBP_direct with flagEnd and a free tf on the device: returns (X_all, u_all, τ1, τ2, t_TU (the final
# grid), dV1, dV2, defect, status, iterations, history [6 x maxIter] = (max|defect|, cost, alpha, τ1, τ2, tf)).
function direct_solve_free_tf(ctx::LtoContext, X_all::Matrix{Float64}, u_all::Matrix{Float64}, τ1, τ2, t_TU::Vector{Float64}, nsteps,
                              Isp, MU, DU, TU, X0_times::Vector{Float64}, X0_states::Matrix{Float64}, Xf_times::Vector{Float64},
                              Xf_states::Matrix{Float64}, flagEnd::Bool, β, tfb::LtoDirectTfBounds, mass, dV1, dV2, maxIter::Integer;
                              allowImpulsive::Bool = false)
    nstate, n_nodes = size(X_all)
    Xo = zeros(nstate, n_nodes); Uo = zeros(3, n_nodes); dV = zeros(6); to = zeros(n_nodes); defect = zeros(nstate, n_nodes - 1)
    tau = [Float64(τ1), Float64(τ2)]; tau_o = zeros(2)
    status = zeros(Cint, 1); iters = zeros(Cint, 1); hist = fill(NaN, 6, max(maxIter, 1))
    prm = Ref(LtoDirectParams(MU, DU, TU, Isp))
    tg = Ref(LtoDirectTargets(zeros(6), zeros(6), mass, dV1, dV2))
    rc = GC.@preserve X0_times X0_states Xf_times Xf_states begin
        ob = Ref(_orbits(X0_times, X0_states, Xf_times, Xf_states))
        ccall(entry(ctx, :direct_solve_free_tf), Cint,
              (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ref{LtoDirectParams}, Ref{LtoDirectOrbits},
               Ref{LtoDirectTargets}, Ptr{Cdouble}, Cdouble, Ref{LtoDirectTfBounds}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble},
               Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}),
              ctx.handle, nstate, n_nodes, X_all, u_all, t_TU, nsteps, prm, ob, tg, tau, β, Ref(tfb), flagEnd, allowImpulsive, maxIter,
              Xo, Uo, dV, to, defect, tau_o, status, iters, hist)
    end
    check(ctx, rc)
    (Xo, Uo, tau_o[1], tau_o[2], to, dV[1:3], dV[4:6], defect, Int(status[1]), Int(iters[1]), hist[:, 1:maxIter])
end

# The operands stay in HBM between calls (struct-of-arrays, see include/lto.h "device-resident API"); every function
# below takes RAW DEVICE POINTERS (`Ptr{Cvoid}`) and a `hipStream_t` (`Ptr{Cvoid}`, C_NULL = HIP's default stream) and
# returns as soon as the work is enqueued.  With AMDGPU.jl: `p = Ptr{Cvoid}(UInt(pointer(A)))` for a `ROCArray{Float64}`
# `A`, `AMDGPU.stream()` for the stream; without it, device memory can come from any HIP allocation in the process.
# This is how a Julia Newton loop keeps the trajectory on the GPU: pack once (`pack_soa!`), then per iteration
# `indirect_jacobian_dev!` -> `newton_solve_dev!` -> `axpy_dev!` -> `indirect_defect_dev!` -> `defect_norms!`, copying two
# scalars per trajectory back.  ctypes twins (executed by the GPU tests): hotpath.IndirectPlan / DirectPlan / pack_soa /
# unpack_soa / defect_norms / Comm / Context.pinned_empty.
const DevPtr = Ptr{Cvoid}
devptr(p::Ptr) = convert(Ptr{Cvoid}, p)
devptr(p::Integer) = Ptr{Cvoid}(UInt(p))
devptr(::Nothing) = C_NULL

"hipStream_t owned by the context (non-blocking); pass it as `stream` to keep library work off the default stream."
ctx_stream(ctx::LtoContext) = ccall((:lto_ctx_stream, liblto), Ptr{Cvoid}, (Ptr{Cvoid},), ctx.handle)
"Wall time [ms] of the last host-pointer call on `ctx`, entry to return, as measured inside the library."
last_call_ms(ctx::LtoContext) = ccall((:lto_last_call_ms, liblto), Cdouble, (Ptr{Cvoid},), ctx.handle)
"Lane order of the last host-pointer indirect call: 0 natural, 1 global, 2 windowed."
last_call_order(ctx::LtoContext) = Int(ccall((:lto_last_call_order, liblto), Cint, (Ptr{Cvoid},), ctx.handle))

"Measure the cost table LTO_KERNEL_AUTO chooses the RK4 STM kernel family by (microseconds per round) on this context's device."
calibrate_kernels!(ctx::LtoContext) = check(ctx, ccall((:lto_calibrate_kernels, liblto), Cint, (Ptr{Cvoid},), ctx.handle))

"Microseconds per round (256 x CUs segments, 64 steps) of the whole-segment lanes (LTO_KERNEL_LANE, 12-dim): the default or this device's (calibrate_kernels!)."
kernel_lane_round_us(ctx::LtoContext) = ccall((:lto_kernel_lane_round_us, liblto), Cdouble, (Ptr{Cvoid},), ctx.handle)

"(`[pipeline8, pipeline48 with 48 segments per workgroup, per-lane, pipeline48 with 44, pipeline32]` microseconds per round at 64 steps, calibrated?) for `ndim` = 12 or 14."
function kernel_round_costs(ctx::LtoContext, ndim::Integer)
    us = zeros(Float64, 5)
    cal = Ref{Cint}(0)
    check(ctx, ccall((:lto_kernel_round_costs, liblto), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cint}), ctx.handle, ndim, us, cal))
    return us, cal[] != 0
end

"""`Array{Float64}` of the given size in page-locked host memory (lto_host_alloc): the GPU reads and writes such arrays (and
contiguous views into them) in place during a host-pointer call -- no copy is queued (Jacobian call at 4 096 segments: 0.20 ms
instead of 0.29 ms with ordinary arrays).  Freed by a finalizer, which may run before or after the context's: the library finds
the block's owner by itself (ctx = NULL) and a context whose destroy was deferred goes with its last block (lto.h, lifetime)."""
function pinned_array(ctx::LtoContext, dims::Integer...)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ctx, ccall((:lto_host_alloc, liblto), Cint, (Ptr{Cvoid}, Csize_t, Ref{Ptr{Cvoid}}), ctx.handle, 8 * prod(dims), p))
    A = unsafe_wrap(Array, convert(Ptr{Float64}, p[]), dims; own = false)
    blk = p[]
    finalizer(_ -> ccall((:lto_host_free, liblto), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), C_NULL, blk), A)
    A
end

"""lto_indirect_plan: per-trajectory parameters uploaded once, then repeated asynchronous sweeps.  `params` = one tuple or a
vector of n_batch tuples (homotopy levels, line-search trial points).  The plan keeps its context alive (lto.h, lifetime)."""
mutable struct LtoIndirectPlan
    handle::Ptr{Cvoid}
    ctx::LtoContext
    ndim::Int; n_nodes::Int; n_batch::Int
    function LtoIndirectPlan(ctx::LtoContext, ndim::Integer, n_nodes::Integer, n_batch::Integer, params; integ::LtoIntegrator = LtoIntegrator())
        prm = params isa Tuple ? [LtoParams(params)] : [LtoParams(q) for q in params]
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(ctx, ccall((:lto_indirect_plan_create, liblto), Cint,
                         (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{LtoParams}, Cint, Ref{LtoIntegrator}, Ref{Ptr{Cvoid}}),
                         ctx.handle, ndim, n_nodes, n_batch, prm, length(prm), Ref(integ), h))
        pl = new(h[], ctx, ndim, n_nodes, n_batch)
        finalizer(q -> (q.handle == C_NULL || ccall((:lto_indirect_plan_destroy, liblto), Cvoid, (Ptr{Cvoid},), q.handle); q.handle = C_NULL), pl)
        pl
    end
end
nseg(pl::LtoIndirectPlan) = (pl.n_nodes - 1) * pl.n_batch

"defect[c*ldd + s] (SoA) of every segment; X[c*ldx + j], t[g*n_nodes + k] on the device.  Replaces indirect.jl:63-90."
function indirect_defect_dev!(pl::LtoIndirectPlan, stream, X, ldx::Integer, t, n_tgrids::Integer, defect, ldd::Integer; errors = nothing)
    check(pl.ctx, ccall((:lto_indirect_defect_dev, liblto), Cint,
                        (Ptr{Cvoid}, Ptr{Cvoid}, DevPtr, Clong, DevPtr, Cint, DevPtr, Clong, DevPtr),
                        pl.handle, devptr(stream), devptr(X), ldx, devptr(t), n_tgrids, devptr(defect), ldd, devptr(errors)))
end

"Phi[(col*ndim+row)*ldp + s] and (optionally) the defect.  Replaces indirect.jl:93-146 (compact blocks)."
function indirect_jacobian_dev!(pl::LtoIndirectPlan, stream, X, ldx::Integer, t, n_tgrids::Integer, Phi, ldp::Integer; defect = nothing, ldd::Integer = 0)
    check(pl.ctx, ccall((:lto_indirect_jacobian_dev, liblto), Cint,
                        (Ptr{Cvoid}, Ptr{Cvoid}, DevPtr, Clong, DevPtr, Cint, DevPtr, Clong, DevPtr, Clong),
                        pl.handle, devptr(stream), devptr(X), ldx, devptr(t), n_tgrids, devptr(Phi), ldp, devptr(defect), ldd))
end

"delta = -Jac_full \\ defect on the device (indirect.jl:181-182; `Phi = nothing` re-uses the factorisation: the SOC re-solve :190-214)."
function newton_solve_dev!(pl::LtoIndirectPlan, stream, Phi, ldp::Integer, defect, ldd::Integer, delta, ldx::Integer; adjoints_only::Bool = false)
    check(pl.ctx, ccall((:lto_indirect_newton_solve_dev, liblto), Cint,
                        (Ptr{Cvoid}, Ptr{Cvoid}, DevPtr, Clong, DevPtr, Clong, Cint, DevPtr, Clong),
                        pl.handle, devptr(stream), devptr(Phi), ldp, devptr(defect), ldd, adjoints_only ? 1 : 0, devptr(delta), ldx))
end

"y = x + alpha d over `count` doubles on the device (trial points, update accumulation)."
axpy_dev!(ctx::LtoContext, stream, x, d, alpha::Real, y, count::Integer) =
    check(ctx, ccall((:lto_axpy_dev, liblto), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, DevPtr, DevPtr, Cdouble, DevPtr, Clong),
                     ctx.handle, devptr(stream), devptr(x), devptr(d), alpha, devptr(y), count))

"The `n_alpha` trial trajectories X + alphas[a] * delta of every trajectory of a batch in one launch (lineSearch, indirect.jl:227-233); `alphas` is a device array."
trial_points_dev!(ctx::LtoContext, stream, X, delta, ld::Integer, ndim::Integer, n_nodes::Integer, n_batch::Integer, n_alpha::Integer, alphas, Xt, ldt::Integer) =
    check(ctx, ccall((:lto_trial_points_dev, liblto), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, DevPtr, DevPtr, Clong, Cint, Cint, Cint, Cint, DevPtr, DevPtr, Clong),
                     ctx.handle, devptr(stream), devptr(X), devptr(delta), ld, ndim, n_nodes, n_batch, n_alpha, devptr(alphas), devptr(Xt), ldt))

"A few device scalars to a host `Vector{Float64}` (`out[1:na] <- a`, `out[na+1:na+nb] <- b`), back when they have arrived: the per-iteration read-back of a Newton loop."
function read_scalars_dev!(ctx::LtoContext, stream, a, na::Integer, b, nb::Integer, out::Vector{Float64})
    # the library copies na + nb doubles to `out`: a short vector would be a heap overwrite
    (na >= 0 && nb >= 0 && length(out) >= na + nb) || throw(ArgumentError("read_scalars_dev!: out needs at least na + nb = $(na + nb) elements"))
    check(ctx, ccall((:lto_read_scalars_dev, liblto), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, DevPtr, Cint, DevPtr, Cint, Ptr{Cdouble}),
                     ctx.handle, devptr(stream), devptr(a), na, devptr(b), nb, out))
end

"lineSearch's first minimiser per trajectory on the device (indirect.jl:244-245): step <- alpha, maxabs_out <- the chosen trial's max |defect|, defect <- its defect block (the check of :328-331 without another sweep)."
line_search_pick_dev!(ctx::LtoContext, stream, sumsq, maxabs, alphas, n_alpha::Integer, trial_defect, ldt::Integer, ndim::Integer, seg_per_traj::Integer, n_batch::Integer, step, maxabs_out, defect, ldd::Integer) =
    check(ctx, ccall((:lto_line_search_pick_dev, liblto), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, DevPtr, DevPtr, DevPtr, Cint, DevPtr, Clong, Cint, Cint, Cint, DevPtr, DevPtr, DevPtr, Clong),
                     ctx.handle, devptr(stream), devptr(sumsq), devptr(maxabs), devptr(alphas), n_alpha, devptr(trial_defect), ldt, ndim, seg_per_traj, n_batch, devptr(step), devptr(maxabs_out), devptr(defect), ldd))

"Order the lanes of the following adaptive sweeps by the last sweep's step counts (results unchanged)."
rebalance!(pl::LtoIndirectPlan, stream) = check(pl.ctx, ccall((:lto_indirect_plan_rebalance, liblto), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), pl.handle, devptr(stream)))
"`(kind, order)`: the lane order the plan's next adaptive sweep would use; kind 0 natural (`order` untouched), 1 global, 2 windowed. `order` needs (n_nodes - 1) * n_batch elements; entries are 0-based segment indices."
function copy_order!(pl::LtoIndirectPlan, stream, order::Vector{Cint})
    kind = Ref{Cint}(-1)
    check(pl.ctx, ccall((:lto_indirect_plan_copy_order, liblto), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cint}, Ptr{Cint}), pl.handle, devptr(stream), order, kind))
    (Int(kind[]), order)
end
"The lane order of the adaptive sweeps for step counts of the caller's choosing (device Cint arrays): kind 1 global, 2 windowed with `weave` windows interleaved (0: the kernel's choice). Read-only; returns when done."
segment_order_dev!(ctx::LtoContext, kind::Integer, weave::Integer, n_segments::Integer, accepted, rejected, order, stream) =
    check(ctx, ccall((:lto_segment_order_dev, liblto), Cint, (Ptr{Cvoid}, Cint, Cint, Cint, DevPtr, DevPtr, DevPtr, Ptr{Cvoid}),
                     ctx.handle, kind, weave, n_segments, devptr(accepted), devptr(rejected), devptr(order), devptr(stream)))
"`out[1:3] <- [sum, max, n_segments]` of accepted + rejected (device Cint arrays), as the defect sweeps' step statistics report them."
function step_stats_dev!(ctx::LtoContext, n_segments::Integer, accepted, rejected, out::Vector{Int64}, stream)
    length(out) >= 3 || throw(ArgumentError("step_stats_dev!: out needs at least 3 elements"))
    check(ctx, ccall((:lto_step_stats_dev, liblto), Cint, (Ptr{Cvoid}, Cint, DevPtr, DevPtr, Ptr{Int64}, Ptr{Cvoid}),
                     ctx.handle, n_segments, devptr(accepted), devptr(rejected), out, devptr(stream)))
    out
end
"LTO_KERNEL_*: 0 auto, 1 per-lane, 2 cooperative, 5 eight-wave pipeline (RK4 plans), 6 cooperative with two lanes per state (12-dim DOP853 plans), 7 pipeline for large batches, 8 32-segment pipeline, 9 whole-segment lanes (RK4 plans); 3 = the direct plans' pipelined Jacobian kernel."
set_kernel!(pl::LtoIndirectPlan, kernel::Integer) = check(pl.ctx, ccall((:lto_indirect_plan_set_kernel, liblto), Cint, (Ptr{Cvoid}, Cint), pl.handle, kernel))
"Family LTO_KERNEL_AUTO resolves to for an STM sweep of this shape on a device with `n_cus` compute units (MI355X cost table): LTO_KERNEL_* (no GPU needed)."
function auto_kernel(ndim::Integer, method::Integer, steps::Integer, p::Real, n_segments::Integer; n_cus::Integer = 256, ordered::Bool = false)
    k = ccall((:lto_indirect_auto_kernel, liblto), Cint, (Cint, Cint, Cint, Cdouble, Clong, Cint, Cint), ndim, method, steps, p, n_segments, n_cus, ordered ? 1 : 0)
    k >= 0 || error("lto_indirect_auto_kernel: invalid shape (code $k)")
    Int(k)
end
"Adaptive sweeps start every segment from its first accepted step size of the plan's previous sweep of the same kind (12-dim DOP853 plans; lto.h)."
set_warm_start!(pl::LtoIndirectPlan, on::Bool = true) = check(pl.ctx, ccall((:lto_indirect_plan_set_warm_start, liblto), Cint, (Ptr{Cvoid}, Cint), pl.handle, on ? 1 : 0))
"Output layout of the plan's sweeps: 0 = struct of arrays, 1 = one block per segment (defect [S][ndim], Phi [S][ndim*ndim] column-major: Julia's own layout; 12-dim DOP853 plans)."
set_output_layout!(pl::LtoIndirectPlan, layout::Integer) = check(pl.ctx, ccall((:lto_indirect_plan_set_output_layout, liblto), Cint, (Ptr{Cvoid}, Cint), pl.handle, layout))
"Record staging of the plan's ordered sweeps, a bit mask: 1 node / defect records in place, 2 Phi records too, 4 an allocation failed and staging is off (lto.h)."
plan_staging(pl::LtoIndirectPlan) = Int(ccall((:lto_indirect_plan_staging, liblto), Cint, (Ptr{Cvoid},), pl.handle))
"STM columns per lane of the per-lane RK4 kernel: 0 auto, 1 or 3 (12-dim) / 1 or 2 (14-dim), or the plan's dimension (12 / 14) = the whole STM in the segment's lane (one-step plans)."
set_cols_per_lane!(pl::LtoIndirectPlan, cols::Integer) = check(pl.ctx, ccall((:lto_indirect_plan_set_cols_per_lane, liblto), Cint, (Ptr{Cvoid}, Cint), pl.handle, cols))
"Lanes per segment of the defect-only sweep of a 12-dim DOP853 plan: 0 = choose (four up to 131 072 segments, then two, then one), 1, 2 or 4."
set_defect_lanes!(pl::LtoIndirectPlan, lanes::Integer = 0) = check(pl.ctx, ccall((:lto_indirect_plan_set_defect_lanes, liblto), Cint, (Ptr{Cvoid}, Cint), pl.handle, lanes))

"Julia column-major [ndim x count] on the device -> SoA [ndim][ld] (and back)."
pack_soa!(ctx::LtoContext, stream, aos, ndim::Integer, count::Integer, soa, ld::Integer) =
    check(ctx, ccall((:lto_pack_soa_dev, liblto), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, DevPtr, Cint, Clong, DevPtr, Clong),
                     ctx.handle, devptr(stream), devptr(aos), ndim, count, devptr(soa), ld))
unpack_soa!(ctx::LtoContext, stream, soa, ld::Integer, ndim::Integer, count::Integer, aos) =
    check(ctx, ccall((:lto_unpack_soa_dev, liblto), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, DevPtr, Clong, Cint, Clong, DevPtr),
                     ctx.handle, devptr(stream), devptr(soa), ld, ndim, count, devptr(aos)))

"sumsq[b] = sum(defect_b.^2) (indirect.jl:240), maxabs[b] = norm(defect_b[:], Inf) (:331) on the device."
defect_norms!(ctx::LtoContext, stream, defect, ldd::Integer, ndim::Integer, seg_per_traj::Integer, n_batch::Integer, sumsq, maxabs) =
    check(ctx, ccall((:lto_defect_norms_dev, liblto), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, DevPtr, Clong, Cint, Cint, Cint, DevPtr, DevPtr),
                     ctx.handle, devptr(stream), devptr(defect), ldd, ndim, seg_per_traj, n_batch, devptr(sumsq), devptr(maxabs)))

mutable struct LtoDirectPlan
    handle::Ptr{Cvoid}
    ctx::LtoContext
    function LtoDirectPlan(ctx::LtoContext, nstate::Integer, n_nodes::Integer, n_batch::Integer, nsteps::Integer, MU, DU, TU, Isp)
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(ctx, ccall((:lto_direct_plan_create, liblto), Cint, (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Ref{LtoDirectParams}, Ref{Ptr{Cvoid}}),
                         ctx.handle, nstate, n_nodes, n_batch, nsteps, Ref(LtoDirectParams(MU, DU, TU, Isp)), h))
        pl = new(h[], ctx)
        finalizer(q -> (q.handle == C_NULL || ccall((:lto_direct_plan_destroy, liblto), Cvoid, (Ptr{Cvoid},), q.handle); q.handle = C_NULL), pl)
        pl
    end
end

"Replaces direct.jl:66-109 with operands in HBM: X[c*ldx + j], U[c*ldu + j] (N), t; defect[c*ldd + s], errors[s]."
function direct_defect_dev!(pl::LtoDirectPlan, stream, X, ldx::Integer, U, ldu::Integer, t, n_tgrids::Integer, defect, ldd::Integer; errors = nothing)
    check(pl.ctx, ccall((:lto_direct_defect_dev, liblto), Cint,
                        (Ptr{Cvoid}, Ptr{Cvoid}, DevPtr, Clong, DevPtr, Clong, DevPtr, Cint, DevPtr, Clong, DevPtr),
                        pl.handle, devptr(stream), devptr(X), ldx, devptr(U), ldu, devptr(t), n_tgrids, devptr(defect), ldd, devptr(errors)))
end

"Replaces direct.jl:111-166 + :503-516: Jac[(col*nstate+row)*ldj + s], dtf[c*ldd + s], defect, errors."
function direct_jacobian_dev!(pl::LtoDirectPlan, stream, X, ldx::Integer, U, ldu::Integer, t, n_tgrids::Integer, Jac, ldj::Integer;
                              dtf = nothing, defect = nothing, ldd::Integer = 0, errors = nothing)
    check(pl.ctx, ccall((:lto_direct_jacobian_dev, liblto), Cint,
                        (Ptr{Cvoid}, Ptr{Cvoid}, DevPtr, Clong, DevPtr, Clong, DevPtr, Cint, DevPtr, Clong, DevPtr, DevPtr, Clong, DevPtr),
                        pl.handle, devptr(stream), devptr(X), ldx, devptr(U), ldu, devptr(t), n_tgrids, devptr(Jac), ldj, devptr(dtf),
                        devptr(defect), ldd, devptr(errors)))
end

# ------------------------------------------------------------------------------------------- collectives (RCCL)
# One Julia process (Distributed worker / MPI rank) per GPU: rank 0 calls comm_unique_id(), ships the 128 bytes to every
# rank (MPI.Bcast!, a RemoteChannel, a file), every rank builds LtoComm(ctx, world, rank, id).  allgather_dev! gives every
# rank the full defect vector, allreduce_dev! its norms -- device to device, nothing returns to the host in between.
function comm_unique_id()
    id = zeros(UInt8, 128)
    rc = ccall((:lto_comm_unique_id, liblto), Cint, (Ptr{UInt8},), id)
    rc == 0 || error("lto_comm_unique_id failed with code $rc (no RCCL in the process?)")
    id
end

mutable struct LtoComm
    handle::Ptr{Cvoid}
    ctx::LtoContext
    world::Int; rank::Int
    function LtoComm(ctx::LtoContext, world::Integer, rank::Integer, id::Vector{UInt8})
        h = Ref{Ptr{Cvoid}}(C_NULL)
        rc = ccall((:lto_comm_create, liblto), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{UInt8}, Ref{Ptr{Cvoid}}), ctx.handle, world, rank, id, h)
        rc == 0 || error("lto_comm_create failed with code $rc")
        LtoComm(h[], ctx, world, rank)
    end
    function LtoComm(handle::Ptr{Cvoid}, ctx::LtoContext, world::Integer, rank::Integer)
        c = new(handle, ctx, world, rank)
        finalizer(q -> (q.handle == C_NULL || ccall((:lto_comm_destroy, liblto), Cvoid, (Ptr{Cvoid},), q.handle); q.handle = C_NULL), c)
        c
    end
end
"""The window transport (lto_comm_window_*): device copies into IPC-mapped receive windows -- no RCCL, no compute units for the
payload, and the one that works for ranks sharing a device.  `exchange(handle::Vector{UInt8}) -> Vector{UInt8}` of world x 128 bytes in
rank order is the launcher's all-gather (MPI.Allgather, a RemoteChannel, files)."""
function LtoCommWindows(ctx::LtoContext, world::Integer, rank::Integer, max_count::Integer, exchange)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    blob = zeros(UInt8, 128)
    rc = ccall((:lto_comm_window_export, liblto), Cint, (Ptr{Cvoid}, Cint, Cint, Clong, Ptr{UInt8}, Ref{Ptr{Cvoid}}), ctx.handle, world, rank, max_count, blob, h)
    rc == 0 || error("lto_comm_window_export failed with code $rc")
    c = LtoComm(h[], ctx, world, rank)
    all = exchange(blob)
    length(all) == 128 * world || error("exchange must return world x 128 bytes in rank order")
    comm_check(c, ccall((:lto_comm_window_open, liblto), Cint, (Ptr{Cvoid}, Ptr{UInt8}), c.handle, all))
    c
end
comm_check(c::LtoComm, rc::Cint) = rc == 0 || error("lto_comm error $rc: " * unsafe_string(ccall((:lto_comm_last_error, liblto), Cstring, (Ptr{Cvoid},), c.handle)))

"recv [world][count] <- send [count] of every rank (device pointers), asynchronous on `stream`."
allgather_dev!(c::LtoComm, stream, send, recv, count::Integer) =
    comm_check(c, ccall((:lto_comm_allgather_dev, liblto), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, DevPtr, DevPtr, Clong), c.handle, devptr(stream), devptr(send), devptr(recv), count))
"buf [count] <- sum (op = 0) or max (op = 1) over ranks, in place."
allreduce_dev!(c::LtoComm, stream, buf, count::Integer, op::Integer) =
    comm_check(c, ccall((:lto_comm_allreduce_dev, liblto), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, DevPtr, Clong, Cint), c.handle, devptr(stream), devptr(buf), count, op))

"True once a wait of a window communicator has run out or the ranks have lost step (every collective since returned NaN); waits for `stream`."
function comm_failed(c::LtoComm, stream)
    f = Ref{Cint}(0)
    comm_check(c, ccall((:lto_comm_status, liblto), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cint}), c.handle, devptr(stream), f))
    f[] != 0
end
"Polls (~1.5 us each) before a wait for a peer gives up and poisons the result."
set_wait_limit!(c::LtoComm, polls::Integer) = comm_check(c, ccall((:lto_comm_set_wait_limit, liblto), Cint, (Ptr{Cvoid}, Clong), c.handle, polls))
"Window transport: payloads of up to `bytes` per rank travel by the push / collect kernels, larger ones by the copy engines (lto.h)."
set_kernel_payload!(c::LtoComm, bytes::Integer) = comm_check(c, ccall((:lto_comm_set_kernel_payload, liblto), Cint, (Ptr{Cvoid}, Clong), c.handle, bytes))
"Ranks RCCL itself reports for this communicator (ncclCommCount); 0 for a window communicator."
function rccl_ranks(c::LtoComm)
    n = ccall((:lto_comm_rccl_ranks, liblto), Cint, (Ptr{Cvoid},), c.handle)
    n >= 0 || error("lto_comm_rccl_ranks failed with code $n")
    Int(n)
end

end # module
