# SLAMHip.jl -- Julia 1.x binding of libslamhip.so (include/slamhip.h).
#
# Keeps the public surface of SLAM.jl's filter core (src/SLAM.jl:5-30: SlamState,
# EKFSlamState, predict, update, add_features, associate, compute_association,
# predict_observation, mpi_to_pi) and adds the in-place names ekf_predict!,
# ekf_update!, augment!.  Every numeric operation is a `ccall` into the HIP
# library; the state lives on the GPU for the life of the handle.
#
# NOTE: there is no `julia` binary in the build image, so this file is written to
# be thin and mechanical and is NOT executed by the test-suite; the same C ABI is
# exercised through the ctypes mirror in ekf.py.  The reference itself is Julia
# 0.5/0.6 syntax (`type`, `atan2`, `chol`) and does not parse on Julia >= 1.0.
module SLAMHip

export SlamState, EKFSlamState, set_state!, predict, update, add_features, associate,
       compute_association, predict_observation, mpi_to_pi,
       ekf_predict!, ekf_update!, augment!, observe!, cov_block, cov_diag, landmark_blocks, gate_mode!, gate_info, state_written!, remove_features!, find_duplicates, merge_landmarks!, transform!, join!, submap, select, reserve!, capacity, associate_joint, observe_joint!, joint_nis, chi2_table, feature_ellipses, vehicle_ellipse,
       PFSlamState, set_pose!, init_landmarks!, pf_predict!, update_known!, step!, step_async!, step_async_batch!, step_unknown!, LandmarkEvidence, evidence_update!, counters, step_unknown_pruned!, flush!,
       PathHistory, record!, path_info, path_record, trace, best_path, mean_path, survivors,
       resample!, mean_pose, weights, particles, pf_map, pf_best_particle, to_ekf, to_particles, peer_blob, attach_peers!, peer_selftest, detach_peers!, comm_info,
       upload!, resize, pose_bins, kld_particle_count, pf_meta, set_rng!,
       CovFactor, factor, factor!, logdet, isposdef, whiten, nees, sample,
       update_linear!, linear_nis, predict_linear!, predict_odometry!, fix_position!, fix_heading!, fix_landmark!,
       step_proposal_unknown!, associate_proposal, proposal_max_obs,
       LocalArea, open_area!, close!, abort!, landmarks_within, accumulators, area_info, global_ids, local_state,
       update_iterated!, iterated_nis, observe_iterated!, iterated_limits,
       FirstEstimates, fej, predict!, update!, reset!, remap!, linearisation, set_linearisation!, fej_limits,
       update_joint!, wide_limits

const libslamhip = get(ENV, "SLAMHIP_LIB", joinpath(@__DIR__, "libslamhip.so"))
# the companion library of include/slamhip_frame.h (the rigid frame change); it links against libslamhip.so and lies beside it
# (opened at the first transform!; it is linked against the libslamhip.so beside it: with SLAMHIP_LIB pointing at another build,
#  point SLAMHIP_FRAME_LIB at a companion linked against THAT build, or do not call transform!)
const libslamhip_frame = get(ENV, "SLAMHIP_FRAME_LIB", joinpath(@__DIR__, "libslamhip_frame.so"))
# the companion library of include/slamhip_join.h (map joining), same arrangement (opened at the first join!)
const libslamhip_join = get(ENV, "SLAMHIP_JOIN_LIB", joinpath(@__DIR__, "libslamhip_join.so"))
# the companion library of include/slamhip_evidence.h (landmark evidence and pruning of the unknown-correspondence particle
# filter), same arrangement (opened at the first LandmarkEvidence)
const libslamhip_evidence = get(ENV, "SLAMHIP_EVIDENCE_LIB", joinpath(@__DIR__, "libslamhip_evidence.so"))
# the companion library of include/slamhip_jc.h (joint-compatibility data association for the EKF), same arrangement (opened at the
# first associate_joint / joint_nis)
const libslamhip_jc = get(ENV, "SLAMHIP_JC_LIB", joinpath(@__DIR__, "libslamhip_jc.so"))
# the companion library of include/slamhip_path.h (per-particle trajectory history of the particle filter), same arrangement
# (opened at the first PathHistory)
const libslamhip_path = get(ENV, "SLAMHIP_PATH_LIB", joinpath(@__DIR__, "libslamhip_path.so"))
# the companion library of include/slamhip_copy.h (an EKF state copied, grown or extracted between two handles), same arrangement
# (opened at the first copy / select / reserve! / capacity)
const libslamhip_copy = get(ENV, "SLAMHIP_COPY_LIB", joinpath(@__DIR__, "libslamhip_copy.so"))
# the companion library of include/slamhip_handover.h (a state handed between the particle filter and the EKF), same arrangement
# (opened at the first to_ekf / to_particles)
const libslamhip_handover = get(ENV, "SLAMHIP_HANDOVER_LIB", joinpath(@__DIR__, "libslamhip_handover.so"))

# the companion library of include/slamhip_pfcopy.h (a particle set uploaded, copied, selected and resized between handles), same
# arrangement (opened at the first copy / select / resize / reserve! / upload! / pose_bins of a particle filter)
const libslamhip_pfcopy = get(ENV, "SLAMHIP_PFCOPY_LIB", joinpath(@__DIR__, "libslamhip_pfcopy.so"))
# the extension library of include/ext/slamhip_factor.h (the Cholesky factor of an EKF state's covariance), same arrangement
# (opened at the first CovFactor)
const libslamhip_factor = get(ENV, "SLAMHIP_FACTOR_LIB", joinpath(@__DIR__, "libslamhip_factor.so"))
# the extension library of include/ext/slamhip_linear.h (caller-supplied motion and measurement models for the EKF), same
# arrangement (opened at the first update_linear! / linear_nis / predict_linear! / predict_odometry!)
const libslamhip_linear = get(ENV, "SLAMHIP_LINEAR_LIB", joinpath(@__DIR__, "libslamhip_linear.so"))
# the extension library of include/ext/slamhip_proposal.h (FastSLAM 2.0 with unknown correspondences), same arrangement (opened at
# the first step_proposal_unknown! / associate_proposal / proposal_max_obs)
const libslamhip_proposal = get(ENV, "SLAMHIP_PROPOSAL_LIB", joinpath(@__DIR__, "libslamhip_proposal.so"))
# the extension library of include/ext/slamhip_local.h (compressed local-area updates for the EKF), same arrangement (opened at the
# first LocalArea; it also needs libslamhip_copy.so beside it)
const libslamhip_local = get(ENV, "SLAMHIP_LOCAL_LIB", joinpath(@__DIR__, "libslamhip_local.so"))
# the extension library of include/ext/slamhip_iterated.h (the iterated EKF update, relinearised on the device), same arrangement
# (opened at the first update_iterated! / iterated_nis / iterated_limits)
const libslamhip_iterated = get(ENV, "SLAMHIP_ITERATED_LIB", joinpath(@__DIR__, "libslamhip_iterated.so"))
# the extension library of include/ext/slamhip_fej.h (first-estimates Jacobian predict, update and augment for the EKF), same
# arrangement (opened at the first FirstEstimates / fej_limits)
const libslamhip_fej = get(ENV, "SLAMHIP_FEJ_LIB", joinpath(@__DIR__, "libslamhip_fej.so"))
# the extension library of include/ext/slamhip_wide.h (the joint update of up to 64 observations in one down-date), same arrangement
# (opened at the first update_joint! / joint_nis / wide_limits; it reads a FirstEstimates object and calls nothing of libslamhip_fej.so)
const libslamhip_wide = get(ENV, "SLAMHIP_WIDE_LIB", joinpath(@__DIR__, "libslamhip_wide.so"))

const SLAM_OK = Cint(0)
const SLAM_PF_HALTED = Cint(1)
const SLAM_E_CAPACITY = Cint(-2)
const SLAM_E_NOTPD = Cint(-3)
const SLAM_F32 = Cint(0)
const SLAM_F64 = Cint(1)
const FORM_CHOLESKY = Cint(0)
const FORM_JOSEPH = Cint(1)

last_error() = unsafe_string(ccall((:slam_last_error, libslamhip), Cstring, ()))

function check(rc::Cint)
    rc == SLAM_OK && return nothing
    # the reference raises PosDefException from chol (src/ekf.jl:70) / BoundsError
    error("libslamhip status $(rc): $(last_error())")
end

abstract type SlamState end                       # src/common.jl:22

"""
    EKFSlamState(x, cov; max_landmarks, device=0, grow=false)

Device-resident counterpart of `EKFSlamState{T}` (src/common.jl:25-28).  `T` is
`Float32` or `Float64`.  `state.x` / `state.cov` download on access; assigning them
uploads.  Capacity is fixed at construction (the reference re-allocates `P` per
new feature, src/ekf.jl:108-109) unless `grow = true`: then `augment!`, `observe!`,
`observe_joint!` and `join!` answer a full map by `reserve!(state, max(2 capacity, needed))`
and finish the step in the larger handle.
"""
mutable struct EKFSlamState{T<:Union{Float32,Float64}} <: SlamState
    handle::Ptr{Cvoid}
    device::Int                                   # the device the handle lives on (submap creates its local map there)
    jc::Ptr{Cvoid}                                # the joint-compatibility search workspace (slam_ekf_jc_create), C_NULL until first used
    grow::Bool                                    # a full map moves into a larger handle (reserve!) instead of failing
    gate::Cint                                    # the gate mode set through gate_mode! (-1: never set), applied again by reserve!
    function EKFSlamState{T}(x::AbstractVector, cov::AbstractMatrix;
                             max_landmarks::Integer = max(64, length(x) - 3), device::Integer = 0, grow::Bool = false) where {T}
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:slam_ekf_create, libslamhip), Cint, (Ref{Ptr{Cvoid}}, Cint, Cint, Cint),
                    h, T === Float32 ? SLAM_F32 : SLAM_F64, max_landmarks, device))
        s = new{T}(h[], Int(device), C_NULL, grow, Cint(-1))
        finalizer(s) do st
            getfield(st, :jc) == C_NULL || ccall((:slam_ekf_jc_destroy, libslamhip_jc), Cint, (Ptr{Cvoid},), getfield(st, :jc))   # it borrows the handle: first
            ccall((:slam_ekf_destroy, libslamhip), Cint, (Ptr{Cvoid},), getfield(st, :handle))
        end
        set_state!(s, x, cov)
        return s
    end
end
EKFSlamState(x::AbstractVector{T}, cov::AbstractMatrix; kw...) where {T<:Union{Float32,Float64}} =
    EKFSlamState{T}(x, cov; kw...)

handle(s::EKFSlamState) = getfield(s, :handle)

function nlandmarks(s::EKFSlamState)
    n = Ref{Cint}(0)
    check(ccall((:slam_ekf_num_landmarks, libslamhip), Cint, (Ptr{Cvoid}, Ref{Cint}), handle(s), n))
    Int(n[])
end
Base.length(s::EKFSlamState) = 3 + 2 * nlandmarks(s)

function set_state!(s::EKFSlamState{T}, x::AbstractVector, cov::AbstractMatrix) where {T}
    xv = Vector{T}(x); P = Matrix{T}(cov)                     # column-major, like the C ABI
    n = length(xv)
    size(P) == (n, n) || throw(DimensionMismatch("cov must be n x n"))
    check(ccall((:slam_ekf_set_state, libslamhip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint),
                handle(s), xv, P, n, n))
    s
end

function download(s::EKFSlamState{T}, which::Symbol) where {T}
    n = length(s)
    x = which === :cov ? C_NULL : Vector{T}(undef, n)
    P = which === :x ? C_NULL : Matrix{T}(undef, n, n)
    check(ccall((:slam_ekf_get_state, libslamhip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint),
                handle(s), x, P, n, n))
    which === :x ? x : which === :cov ? P : (x, P)
end

function Base.getproperty(s::EKFSlamState, f::Symbol)
    f === :x && return download(s, :x)
    f === :cov && return download(s, :cov)
    getfield(s, f)
end

function Base.setproperty!(s::EKFSlamState, f::Symbol, v)
    # `state.x, state.cov = predict(state, ...)` (sim/ekfslam-sim.jl:100) hands back `nothing`
    # placeholders from the in-place kernels: nothing to upload.
    v === nothing && return v
    if f === :x
        length(v) == length(s) || error("x and cov change size together: use set_state!(state, x, cov)")
        set_state!(s, v, download(s, :cov))
        return v
    elseif f === :cov
        size(v, 1) == length(s) || error("x and cov change size together: use set_state!(state, x, cov)")
        set_state!(s, download(s, :x), v)
        return v
    end
    setfield!(s, f, v)
end

colmajor4(M::AbstractMatrix) = Float64[M[1, 1], M[2, 1], M[1, 2], M[2, 2]]
pairs64(z::AbstractMatrix) = Matrix{Float64}(z)              # 2 x nz column-major == (range, bearing) pairs

"Single conditional wrap, src/common.jl:102-110."
function mpi_to_pi(phi::AbstractFloat)
    phi > pi && return phi - 2pi
    phi < -pi && return phi + 2pi
    phi
end

# ---- in-place operations ---------------------------------------------------------------
"predict (src/ekf.jl:8-43) in place on the device."
function ekf_predict!(s::EKFSlamState, v::Real, g::Real, wheelbase::Real, Q::AbstractMatrix, dt::Real)
    check(ccall((:slam_ekf_predict, libslamhip), Cint, (Ptr{Cvoid}, Cdouble, Cdouble, Cdouble, Ptr{Cdouble}, Cdouble),
                handle(s), v, g, wheelbase, colmajor4(Q), dt))
    s
end

"update (src/ekf.jl:46-77) in place on the device; `form = :joseph` selects the rank-2k Joseph form."
function ekf_update!(s::EKFSlamState, z::AbstractMatrix, R::AbstractMatrix, idf; form::Symbol = :cholesky)
    m = size(z, 2)
    m == 0 && return s
    ids = Vector{Int32}(vec(collect(idf)))
    check(ccall((:slam_ekf_update, libslamhip), Cint,
                (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Int32}, Cint, Ptr{Cdouble}, Cint),
                handle(s), pairs64(z), ids, m, colmajor4(R), form === :joseph ? FORM_JOSEPH : FORM_CHOLESKY))
    s
end

"add_features (src/ekf.jl:84-122) in place on the device.  A growing state (`grow = true`) that is full reserves room first."
function augment!(s::EKFSlamState, z::AbstractMatrix, R::AbstractMatrix)
    nn = size(z, 2)
    nn == 0 && return s
    call() = ccall((:slam_ekf_augment, libslamhip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Ptr{Cdouble}),
                   handle(s), pairs64(z), nn, colmajor4(R))
    rc = call()
    if rc == SLAM_E_CAPACITY && getfield(s, :grow)          # decided before anything was enqueued: grow, then again
        grow_for!(s, nlandmarks(s) + nn)
        rc = call()
    end
    check(rc)
    s
end

"""
observe!(state, z, R, gate1, gate2; form = :cholesky) -> assoc::Vector{Int32}

The observation step of sim! (sim/ekfslam-sim.jl:114-120: associate, update, add_features) as one
library call with the same results; no host round trip between the gating and the update.
assoc[i] >= 1: matched landmark, 0: dropped, -1: appended as a new feature.
"""
function observe!(s::EKFSlamState, z::AbstractMatrix, R::AbstractMatrix, gate1::Real, gate2::Real;
                  form::Symbol = :cholesky)
    nz = size(z, 2)
    assoc = zeros(Int32, nz)
    nz == 0 && return assoc
    rc = ccall((:slam_ekf_observe, libslamhip), Cint,
               (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cdouble, Cdouble, Cint, Ptr{Int32}),
               handle(s), pairs64(z), nz, colmajor4(R), gate1, gate2, form == :joseph ? 1 : 0, assoc)
    if rc == SLAM_E_CAPACITY && getfield(s, :grow)
        # the association vector is complete and the update has been applied; only the new features are missing
        augment!(s, pairs64(z)[:, assoc .< 0], R)
        return assoc
    end
    check(rc)
    assoc
end

# ---- looking at the covariance without downloading it ------------------------------------------
"cov[r, c] for the ranges r, c (1-based, like `state.cov[r, c]`) without downloading the matrix (slam_ekf_get_block)."
function cov_block(s::EKFSlamState{T}, r::AbstractUnitRange, c::AbstractUnitRange) where {T}
    out = Matrix{T}(undef, length(r), length(c))
    check(ccall((:slam_ekf_get_block, libslamhip), Cint, (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Ptr{Cvoid}, Cint),
                handle(s), first(r) - 1, first(c) - 1, length(r), length(c), out, max(length(r), 1)))
    out
end

"diag(state.cov) (slam_ekf_get_diag)."
function cov_diag(s::EKFSlamState{T}) where {T}
    out = Vector{T}(undef, length(s))
    check(ccall((:slam_ekf_get_diag, libslamhip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), handle(s), out))
    out
end

"The landmarks' 2 x 2 covariance blocks, 3 x N: [P[f,f]; P[f+1,f]; P[f+1,f+1]] per landmark (slam_ekf_get_landmark_blocks)."
function landmark_blocks(s::EKFSlamState{T}) where {T}
    N = div(length(s) - 3, 2)
    out = Matrix{T}(undef, N, 3)                     # the library writes three rows of N values
    check(ccall((:slam_ekf_get_landmark_blocks, libslamhip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), handle(s), out))
    permutedims(out)
end

"""
    gate_mode!(s, mode)    mode in (:auto, :sweep, :grid)

How `associate` / `observe!` search the map -- the TODO of src/data-association.jl:18-20: `:sweep` visits every landmark,
`:grid` keeps a uniform grid over the landmark means on the device and visits only the cells an observation's gate can
reach (O(candidates)), `:auto` (default) takes the grid from 16384 landmarks on.  The decisions are identical.
"""
function gate_mode!(s::EKFSlamState, mode::Symbol)
    m = mode === :auto ? 0 : mode === :sweep ? 1 : mode === :grid ? 2 : throw(ArgumentError("gate mode must be :auto, :sweep or :grid"))
    check(ccall((:slam_ekf_set_gate_mode, libslamhip), Cint, (Ptr{Cvoid}, Cint), handle(s), m))
    setfield!(s, :gate, Cint(m))
    s
end

"slam_ekf_gate_info: (form of the last gating, cells per axis, landmarks in the grid, tail, rebuilds, queries, visited, evaluated)."
function gate_info(s::EKFSlamState)
    out = zeros(Int64, 8)
    check(ccall((:slam_ekf_gate_info, libslamhip), Cint, (Ptr{Cvoid}, Ptr{Int64}), handle(s), out))
    (form = (nothing, :sweep, :grid)[out[1] + 1], cells_per_axis = out[2], in_grid = out[3], tail = out[4],
     rebuilds = out[5], queries = out[6], visited = out[7], evaluated = out[8])
end

"""
    state_written!(s)

After writing landmark entries of `x` / `cov` through raw device views (slam_ekf_device_ptrs): refreshes what the gating
keeps beside the matrix (packed 2 x 2 blocks, variance bound, grid of means).  Assigning `s.x` / `s.cov` needs no call.
"""
function state_written!(s::EKFSlamState)
    check(ccall((:slam_ekf_state_written, libslamhip), Cint, (Ptr{Cvoid},), handle(s)))
    s
end

"""
    remove_features!(s, ids) -> new_index::Vector{Int32}

Map management (no counterpart in the reference, whose map only grows): the landmarks `ids` (1-based, any order) leave the
map in place on the device -- x <- x[keep], cov <- cov[keep, keep], bit for bit; the others keep their order and are
renumbered.  `new_index[j]` is the new id of old landmark j, 0 if it was removed (slam_ekf_remove_landmarks).
"""
function remove_features!(s::EKFSlamState, ids::AbstractVector{<:Integer})
    new_index = zeros(Int32, nlandmarks(s))
    rm = collect(Int32, ids)
    check(ccall((:slam_ekf_remove_landmarks, libslamhip), Cint, (Ptr{Cvoid}, Ptr{Int32}, Cint, Ptr{Int32}),
                handle(s), rm, length(rm), new_index))
    new_index
end

"""
    find_duplicates(s, gate; cap = 1024) -> (pairs::Matrix{Int32}, count)

Landmarks entered twice (slam_ekf_find_duplicates): the pairs (a, b), a < b, whose difference has a Mahalanobis distance below
`gate` under D = P_aa + P_bb - P_ab - P_ab'.  `pairs` is 2 x min(count, cap), one pair per column, ascending; `count` is the
number of pairs in the whole map.  The state is not changed.
"""
function find_duplicates(s::EKFSlamState, gate::Real; cap::Integer = 1024)
    pairs = zeros(Int32, 2, max(cap, 0))
    count = Ref{Cint}(0)
    check(ccall((:slam_ekf_find_duplicates, libslamhip), Cint, (Ptr{Cvoid}, Cdouble, Ptr{Int32}, Cint, Ref{Cint}),
                handle(s), gate, pairs, cap, count))
    pairs[:, 1:min(Int(count[]), max(cap, 0))], Int(count[])
end

"""
    merge_landmarks!(s, pairs; Rc = nothing) -> new_index::Vector{Int32}

Fuse the landmarks of every column (a, b) of `pairs` (2 x cnt, cnt <= 8, no landmark twice) into one: the constraint
m_a - m_b = 0 with noise `Rc` (2 x 2, `nothing` = exact) as one Cholesky-form update, then b leaves the map as
`remove_features!` removes it (slam_ekf_merge_landmarks).  `new_index[j]` is the new id of old landmark j; for a removed b
the new id of its a.
"""
function merge_landmarks!(s::EKFSlamState, pairs::AbstractMatrix{<:Integer}; Rc = nothing)
    size(pairs, 1) == 2 || throw(ArgumentError("pairs must be 2 x cnt"))
    new_index = zeros(Int32, nlandmarks(s))
    pr = collect(Int32, pairs)
    rc = Rc === nothing ? C_NULL : collect(Float64, Rc)      # column-major double[4], as R
    check(ccall((:slam_ekf_merge_landmarks, libslamhip), Cint, (Ptr{Cvoid}, Ptr{Int32}, Cint, Ptr{Cdouble}, Ptr{Int32}),
                handle(s), pr, size(pr, 2), rc, new_index))
    new_index
end

"""
    transform!(s, tx, ty, theta) -> s

Express the whole state in another frame, in place on the device (slam_ekf_transform): every position becomes
R(theta) p + (tx, ty), the heading mpi_to_pi(phi + theta), cov becomes T cov T' with T = blockdiag(R, 1, R, R, ...).  Enqueued.
"""
function transform!(s::EKFSlamState, tx::Real, ty::Real, theta::Real)
    check(ccall((:slam_ekf_transform, libslamhip_frame), Cint, (Ptr{Cvoid}, Cdouble, Cdouble, Cdouble), handle(s), tx, ty, theta))
    s
end

"""
    submap(s, max_landmarks) -> EKFSlamState

A fresh local map for `join!`: same element type and same device as `s`, pose (0, 0, 0), no landmark, cov = 0.  Its frame is the
vehicle pose of `s` for as long as `s` neither moves nor observes.
"""
submap(s::EKFSlamState{T}, max_landmarks::Integer) where {T} =
    EKFSlamState{T}(zeros(T, 3), zeros(T, 3, 3); max_landmarks = max_landmarks, device = getfield(s, :device))

"""
    join!(a, b; merge_gate = nothing, Rc = nothing) -> first_new  |  (first_new, new_index)

Map joining on the device (slam_ekf_join): the local map `b`, whose frame is `a`'s vehicle pose (`submap`), is appended to `a`:
the vehicle is composed with `b`'s, `b`'s landmark j becomes landmark N_a + j, cov becomes F cov F' + G cov_b G'.  `b` is only
read.  `first_new` is the id in `a` of `b`'s first landmark.  With `merge_gate` the overlap is fused afterwards
(`find_duplicates(a, merge_gate)`, then `merge_landmarks!` on at most 8 disjoint pairs, round after round until no pair is found)
and the composed `new_index` (one entry per landmark of the joined map) is returned as well.
"""
function join!(a::EKFSlamState{T}, b::EKFSlamState{T}; merge_gate = nothing, Rc = nothing) where {T}
    first = Ref{Int32}(0)
    call() = ccall((:slam_ekf_join, libslamhip_join), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Int32}), handle(a), handle(b), first)
    rc = call()
    if rc == SLAM_E_CAPACITY && getfield(a, :grow)          # decided before anything was enqueued: grow, then again
        grow_for!(a, nlandmarks(a) + nlandmarks(b))
        rc = call()
    end
    check(rc)
    merge_gate === nothing && return Int(first[])
    cur = collect(Int32, 1:nlandmarks(a))
    while true
        pairs, count = find_duplicates(a, merge_gate)
        count == 0 && break
        batch = Vector{Int32}[]
        busy = Set{Int32}()
        for k in 1:size(pairs, 2)
            length(batch) == 8 && break
            (pairs[1, k] in busy || pairs[2, k] in busy) && continue
            push!(batch, pairs[:, k]); push!(busy, pairs[1, k], pairs[2, k])
        end
        new_index = merge_landmarks!(a, reduce(hcat, batch); Rc = Rc)
        cur = new_index[cur]
    end
    Int(first[]), cur
end

# ---- a state moved between two handles on the device (include/slamhip_copy.h) ---------------------------------------------------
"The landmark capacity of the handle (slam_ekf_capacity)."
function capacity(s::EKFSlamState)
    out = Ref{Cint}(0)
    check(ccall((:slam_ekf_capacity, libslamhip_copy), Cint, (Ptr{Cvoid}, Ref{Cint}), handle(s), out))
    Int(out[])
end

blank(s::EKFSlamState{T}, max_landmarks::Integer) where {T} =
    EKFSlamState{T}(zeros(T, 3), zeros(T, 3, 3); max_landmarks = max_landmarks, device = getfield(s, :device), grow = getfield(s, :grow))

"""
    copy!(dst, src) -> dst

`dst` becomes `src` on the device (slam_ekf_copy): N, x and every entry of cov, bit for bit.  The capacities may differ in either
direction as long as `src`'s landmarks fit `dst`.  `src` is only read.  Enqueued, does not synchronise.
"""
function Base.copy!(dst::EKFSlamState{T}, src::EKFSlamState{T}) where {T}
    check(ccall((:slam_ekf_copy, libslamhip_copy), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), handle(dst), handle(src)))
    dst
end

"    copy(s; max_landmarks = capacity(s)) -> a new state on the same device that holds `s` (`copy!`): a fork to try a hypothesis on."
Base.copy(s::EKFSlamState; max_landmarks::Integer = capacity(s)) = copy!(blank(s, max_landmarks), s)

"""
    select(s, ids; max_landmarks = max(64, 2 length(ids))) -> EKFSlamState

The sub-map `ids` (1-based, distinct, any order; none: the vehicle alone) of `s` with its full marginal covariance, in a new state on
the same device (slam_ekf_select): its landmark k is `s`'s landmark `ids[k]`, x = x[sel], cov = cov[sel, sel], bit for bit.
"""
function select(s::EKFSlamState, ids::AbstractVector{<:Integer}; max_landmarks::Integer = max(64, 2 * length(ids)))
    dst = blank(s, max_landmarks)
    sel = collect(Int32, ids)
    check(ccall((:slam_ekf_select, libslamhip_copy), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}, Cint),
                handle(dst), handle(s), sel, length(sel)))
    dst
end

"""
    reserve!(s, max_landmarks) -> s

Make room for `max_landmarks` landmarks (nothing happens if the capacity is already that large): a new handle is created, the state
is copied into it on the device, it takes the old handle's place inside `s` and the old one is destroyed.  The gate mode set through
`gate_mode!` is applied again; the joint-association workspace is dropped and made again at the next joint call.  Raw device pointers
obtained before are dead afterwards.  Old and new matrix exist side by side during the call.
"""
function reserve!(s::EKFSlamState{T}, max_landmarks::Integer) where {T}
    max_landmarks <= capacity(s) && return s
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:slam_ekf_create, libslamhip), Cint, (Ref{Ptr{Cvoid}}, Cint, Cint, Cint),
                h, T === Float32 ? SLAM_F32 : SLAM_F64, max_landmarks, getfield(s, :device)))
    rc = ccall((:slam_ekf_copy, libslamhip_copy), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), h[], handle(s))
    if rc == SLAM_OK && getfield(s, :gate) >= 0
        rc = ccall((:slam_ekf_set_gate_mode, libslamhip), Cint, (Ptr{Cvoid}, Cint), h[], getfield(s, :gate))
    end
    if rc != SLAM_OK
        ccall((:slam_ekf_destroy, libslamhip), Cint, (Ptr{Cvoid},), h[])
        check(rc)
    end
    if getfield(s, :jc) != C_NULL                            # it borrows the old handle
        ccall((:slam_ekf_jc_destroy, libslamhip_jc), Cint, (Ptr{Cvoid},), getfield(s, :jc))
        setfield!(s, :jc, C_NULL)
    end
    old = handle(s)
    setfield!(s, :handle, h[])
    ccall((:slam_ekf_destroy, libslamhip), Cint, (Ptr{Cvoid},), old)      # (waits for the copy's last read of it)
    s
end

"The growth rule of a growing state: twice the capacity, or what is needed if that is more."
grow_for!(s::EKFSlamState, needed::Integer) = reserve!(s, max(2 * capacity(s), needed))

# ---- the Cholesky factor of cov on the device (include/ext/slamhip_factor.h) ----------------------------------------------------
"""
    CovFactor{T}(max_landmarks; device = 0, panel_tiles = 0)

The Cholesky factor L of an EKF state's covariance on the device, L L' = cov, in arithmetic and storage type `T`, with the snapshot
of x that `factor!` took.  `panel_tiles`: 1, 2 or 4 tile columns per panel, 0 = the default for `T`.
"""
mutable struct CovFactor{T<:Union{Float32,Float64}}
    handle::Ptr{Cvoid}
    function CovFactor{T}(max_landmarks::Integer; device::Integer = 0, panel_tiles::Integer = 0) where {T}
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:slam_ekf_factor_create, libslamhip_factor), Cint, (Ref{Ptr{Cvoid}}, Cint, Cint, Cint, Cint),
                    h, T === Float32 ? SLAM_F32 : SLAM_F64, max_landmarks, device, panel_tiles))
        f = new{T}(h[])
        finalizer(f) do ff
            ccall((:slam_ekf_factor_destroy, libslamhip_factor), Cint, (Ptr{Cvoid},), ff.handle)
        end
        return f
    end
end

"    factor!(f, s) -> (status, info): factor `s`'s covariance into `f` (slam_ekf_factor_compute); SLAM_E_NOTPD is returned, not raised."
function factor!(f::CovFactor, s::EKFSlamState)
    info = zeros(Float64, 8)
    rc = ccall((:slam_ekf_factor_compute, libslamhip_factor), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cdouble}), f.handle, handle(s), info)
    rc == SLAM_OK || rc == SLAM_E_NOTPD || check(rc)
    rc, info
end

"    factor(s; T = eltype of s, panel_tiles = 0) -> CovFactor: cov = L L' on the device; an error when a pivot fails.  Synchronises."
function factor(s::EKFSlamState{S}; T::Type = S, panel_tiles::Integer = 0) where {S}
    f = CovFactor{T}(capacity(s); device = getfield(s, :device), panel_tiles = panel_tiles)
    rc, _ = factor!(f, s)
    check(rc)
    f
end

"[n, status, first failing index (0-based) or -1, failing pivot, min l_ii, max l_ii, log det, panel_tiles] of the last factor!."
function factor_info(f::CovFactor)
    info = zeros(Float64, 8)
    check(ccall((:slam_ekf_factor_info, libslamhip_factor), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), f.handle, info))
    info
end
Base.length(f::CovFactor) = Int(factor_info(f)[1])

"log det cov = 2 sum log l_ii (map entropy up to a constant)."
logdet(f::CovFactor) = factor_info(f)[7]

"""
    isposdef(s; T = Float64) -> (ok, index, landmark)

Whether cov has a Cholesky factor in `T` arithmetic; if not, the first failing state index (1-based) and its landmark (0: the vehicle).
"""
function isposdef(s::EKFSlamState; T::Type = Float64)
    f = CovFactor{T}(capacity(s); device = getfield(s, :device))
    rc, info = factor!(f, s)
    finalize(f)
    rc == SLAM_OK && return (true, 0, 0)
    i = Int(info[3])
    (false, i + 1, i < 3 ? 0 : (i - 3) ÷ 2 + 1)
end

"    L(f, r0, c0, nr, nc): the block L[r0 : r0 + nr - 1, c0 : c0 + nc - 1] (1-based), zeros above the diagonal."
function factor_block(f::CovFactor{T}, r0::Integer, c0::Integer, nr::Integer, nc::Integer) where {T}
    out = Matrix{T}(undef, nr, nc)
    check(ccall((:slam_ekf_factor_get, libslamhip_factor), Cint, (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Ptr{Cvoid}, Cint),
                f.handle, r0 - 1, c0 - 1, nr, nc, out, max(nr, 1)))
    out
end

"x as the last factor! found it, as Float64."
function factor_mean(f::CovFactor)
    x = zeros(Float64, length(f))
    check(ccall((:slam_ekf_factor_mean, libslamhip_factor), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), f.handle, x))
    x
end

"    whiten(f, E) -> (Y, d2): Y = L^-1 E for an n x r matrix of error vectors, r <= 64, and the squared norms of Y's columns (fp64)."
function whiten(f::CovFactor, E::AbstractMatrix)
    B = Matrix{Float64}(E)
    n, r = size(B)
    Y = similar(B)
    d2 = zeros(Float64, r)
    check(ccall((:slam_ekf_factor_solve, libslamhip_factor), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}),
                f.handle, B, r, n, Y, d2))
    Y, d2
end

"    nees(f, x_true): e' cov^-1 e with e = mean - x_true, the heading difference wrapped by mpi_to_pi."
function nees(f::CovFactor, x_true::AbstractVector)
    e = factor_mean(f) .- x_true
    e[3] = mpi_to_pi(e[3])
    whiten(f, reshape(e, :, 1))[2][1]
end

"    sample(f, Z): mean .+ L Z for an n x r matrix Z of the caller's standard normals, r <= 64: joint samples of the state."
function sample(f::CovFactor, Z::AbstractMatrix)
    Zd = Matrix{Float64}(Z)
    n, r = size(Zd)
    out = similar(Zd)
    check(ccall((:slam_ekf_factor_multiply, libslamhip_factor), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}),
                f.handle, Zd, r, n, out))
    factor_mean(f) .+ out
end

# ---- caller-supplied models (include/ext/slamhip_linear.h) ------------------------------------------------------------------------
# H: a k x n matrix (k <= 16 rows of at most 8 non-zeros).  The C interface counts state indices from 0; the Julia matrix's
# column c is state index c - 1.
function linear_rows(H::AbstractMatrix)
    ptr = Cint[0]; idx = Cint[]; val = Float64[]
    for i in 1:size(H, 1)
        for c in 1:size(H, 2)
            H[i, c] == 0 && continue
            push!(idx, c - 1); push!(val, H[i, c])
        end
        push!(ptr, length(idx))
    end
    ptr, idx, val
end

function linear_mask(wrap, innovation::Bool)
    mask = UInt32(0)
    for i in wrap
        mask |= UInt32(1) << (i - 1)                                     # rows are counted from 1 here
    end
    mask, Cint(innovation ? 1 : 0)
end

"""
    update_linear!(s, H, z, R; wrap = (), innovation = false) -> [v' inv(S) v, log det S, smallest pivot, -1]

The Kalman update from a linear measurement z = H x + noise(R), in place on the device (slam_ekf_update_linear).  `wrap`: the
rows (1-based) whose innovation is an angle.  `innovation = true`: `z` already is the innovation.
"""
function update_linear!(s::EKFSlamState, H::AbstractMatrix, z::AbstractVector, R::AbstractMatrix; wrap = (), innovation::Bool = false)
    ptr, idx, val = linear_rows(H)
    mask, mode = linear_mask(wrap, innovation)
    out = zeros(Float64, 4)
    check(ccall((:slam_ekf_update_linear, libslamhip_linear), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, UInt32, Ptr{Cdouble}),
                handle(s), size(H, 1), ptr, idx, val, Vector{Float64}(z), Matrix{Float64}(R), mode, mask, out))
    out
end

"    linear_nis(s, H, z, R; wrap, innovation): what update_linear! would return; the state is only read (the chi-square gate)."
function linear_nis(s::EKFSlamState, H::AbstractMatrix, z::AbstractVector, R::AbstractMatrix; wrap = (), innovation::Bool = false)
    ptr, idx, val = linear_rows(H)
    mask, mode = linear_mask(wrap, innovation)
    out = zeros(Float64, 4)
    check(ccall((:slam_ekf_linear_nis, libslamhip_linear), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, UInt32, Ptr{Cdouble}),
                handle(s), size(H, 1), ptr, idx, val, Vector{Float64}(z), Matrix{Float64}(R), mode, mask, out))
    out
end

"    predict_linear!(s, xv, Gv, Qv): x[1:3] = xv, P_vv = Gv P_vv Gv' + Qv, P_vm = Gv P_vm (slam_ekf_predict_linear)."
function predict_linear!(s::EKFSlamState, xv::AbstractVector, Gv::AbstractMatrix, Qv::AbstractMatrix)
    check(ccall((:slam_ekf_predict_linear, libslamhip_linear), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                handle(s), Vector{Float64}(xv), Matrix{Float64}(Gv), Matrix{Float64}(Qv)))
    nothing
end

"    predict_odometry!(s, d, Q3): compose the pose with the vehicle-frame increment d = (dx, dy, dtheta) of covariance Q3, on the device."
function predict_odometry!(s::EKFSlamState, d::AbstractVector, Q3::AbstractMatrix)
    check(ccall((:slam_ekf_predict_odometry, libslamhip_linear), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}),
                handle(s), Vector{Float64}(d), Matrix{Float64}(Q3)))
    nothing
end

function unit_rows(n::Integer, cols)
    H = zeros(Float64, length(cols), n)
    for (i, c) in enumerate(cols)
        H[i, c] = 1.0
    end
    H
end
"    fix_position!(s, xy, R): the vehicle is at xy with covariance R (a GPS receiver)."
fix_position!(s::EKFSlamState, xy, R) = update_linear!(s, unit_rows(length(s), (1, 2)), xy, R)
"    fix_heading!(s, phi, var): the heading is phi with variance var (a compass); the innovation is wrapped."
fix_heading!(s::EKFSlamState, phi, var) = update_linear!(s, unit_rows(length(s), (3,)), [phi], fill(Float64(var), 1, 1); wrap = (1,))
"    fix_landmark!(s, j, xy, R): landmark j was surveyed at xy with covariance R."
fix_landmark!(s::EKFSlamState, j::Integer, xy, R) = update_linear!(s, unit_rows(length(s), (2 + 2j, 3 + 2j)), xy, R)

# ---- the iterated update (include/ext/slamhip_iterated.h; no counterpart in the reference) ---------------------------------------
"    iterated_limits() -> (observations per call, iterations per call) as libslamhip_iterated.so reports them."
function iterated_limits()
    out = zeros(Int32, 2)
    check(ccall((:slam_ekf_iterated_limits, libslamhip_iterated), Cint, (Ptr{Int32},), out))
    Int(out[1]), Int(out[2])
end

iterated_result(out) = (iterations = Int(out[1]), converged = out[2] != 0, step = out[3], nis = out[4], log_det = out[5],
                        cost_first = out[9], cost_last = out[10], out = out)

"""
    update_iterated!(s, z, R, idf; max_iter = 10, tol = 1e-9) -> (iterations, converged, step, nis, log_det, cost_first, cost_last, out)

The iterated EKF update in place on the device (slam_ekf_update_iterated): `ekf_update!` in its Cholesky form with the range-bearing
model relinearised at every iterate (Gauss-Newton on the MAP cost, WITHOUT a line search) until the largest change of an iterate is
at most `tol` or `max_iter` (1 .. 64) iterations have run.  `max_iter = 1` is `ekf_update!`.  A call takes at most 8 observations; more
are applied as consecutive batches of 8 in the order given, each iterated on the state the batch before left: SEQUENTIAL, not the
joint update of all of them; the result is then the last batch's.  `nothing` for no observation.
"""
function update_iterated!(s::EKFSlamState, z::AbstractMatrix, R::AbstractMatrix, idf; max_iter::Integer = 10, tol::Real = 1e-9)
    m = size(z, 2)
    ids = Vector{Int32}(vec(collect(idf)))
    length(ids) == m || throw(ArgumentError("idf and z disagree on the number of observations"))
    zz, r = pairs64(z), colmajor4(R)
    res = nothing
    for lo in 1:8:m
        hi = min(lo + 7, m)
        out = zeros(Float64, 10)
        check(ccall((:slam_ekf_update_iterated, libslamhip_iterated), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Int32}, Cint, Ptr{Cdouble}, Cint, Cdouble, Ptr{Cdouble}),
                    handle(s), zz[:, lo:hi], ids[lo:hi], hi - lo + 1, r, max_iter, tol, out))
        res = iterated_result(out)
    end
    res
end

"    iterated_nis(s, z, R, idf; max_iter, tol): what update_iterated! would return; the state is only read (the dry run).  At most 8 observations."
function iterated_nis(s::EKFSlamState, z::AbstractMatrix, R::AbstractMatrix, idf; max_iter::Integer = 10, tol::Real = 1e-9)
    m = size(z, 2)
    ids = Vector{Int32}(vec(collect(idf)))
    length(ids) == m || throw(ArgumentError("idf and z disagree on the number of observations"))
    out = zeros(Float64, 10)
    check(ccall((:slam_ekf_iterated_nis, libslamhip_iterated), Cint,
                (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Int32}, Cint, Ptr{Cdouble}, Cint, Cdouble, Ptr{Cdouble}),
                handle(s), pairs64(z), ids, m, colmajor4(R), max_iter, tol, out))
    iterated_result(out)
end

"    observe_iterated!(s, z, R, gate1, gate2; max_iter, tol) -> (assoc, result): associate, update_iterated!, augment! in sequence from the host."
function observe_iterated!(s::EKFSlamState, z::AbstractMatrix, R::AbstractMatrix, gate1::Real, gate2::Real; max_iter::Integer = 10,
                           tol::Real = 1e-9)
    zf, idf, zn = associate(s, z, R, gate1, gate2)
    assoc = zeros(Int32, size(z, 2))
    hit, new = 0, 0
    for i in 1:size(z, 2)                                                # the association vector of observe!, from the two lists
        if hit < size(zf, 2) && z[:, i] == zf[:, hit + 1]
            hit += 1
            assoc[i] = idf[hit]
        elseif new < size(zn, 2) && z[:, i] == zn[:, new + 1]
            new += 1
            assoc[i] = -1
        end
    end
    res = update_iterated!(s, zf, R, idf; max_iter = max_iter, tol = tol)
    augment!(s, zn, R)
    assoc, res
end

# ---- first-estimates Jacobians (include/ext/slamhip_fej.h; no counterpart in the reference) ---------------------------------------
"    fej_limits() -> observations per update call as libslamhip_fej.so reports them."
function fej_limits()
    out = zeros(Int32, 1)
    check(ccall((:slam_ekf_fej_limits, libslamhip_fej), Cint, (Ptr{Int32},), out))
    Int(out[1])
end

"""
    FirstEstimates(s)   (or fej(s))

The linearisation points of a first-estimates Jacobian (FEJ) filter over `s`, on the device beside the state: `lin`, the pose the
vehicle's Jacobians are evaluated at (the predicted pose, never an updated one), and `first`, every landmark's first estimate.
`predict!`, `update!` and `augment!` on this object are `ekf_predict!`, `ekf_update!` (Cholesky form) and `augment!` of `s` with the
Jacobians evaluated there, so that the filter gains no information along the three unobservable directions of the map.  After the map
was renumbered outside the object (remove_features!, merge_landmarks!, join!) it refuses to work until `remap!` was told how.
`s` must outlive the object; `close!(f)` releases it early.
"""
mutable struct FirstEstimates{T<:Union{Float32,Float64}}
    handle::Ptr{Cvoid}
    state::EKFSlamState{T}
    function FirstEstimates(s::EKFSlamState{T}) where {T}
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:slam_ekf_fej_create, libslamhip_fej), Cint, (Ref{Ptr{Cvoid}}, Ptr{Cvoid}), h, handle(s)))
        f = new{T}(h[], s)
        finalizer(close!, f)
        return f
    end
end

fej(s::EKFSlamState) = FirstEstimates(s)

function close!(f::FirstEstimates)
    if f.handle != C_NULL
        ccall((:slam_ekf_fej_destroy, libslamhip_fej), Cint, (Ptr{Cvoid},), f.handle)
        f.handle = C_NULL
    end
    nothing
end

"    predict!(f, v, g, wheelbase, Q, dt): ekf_predict! with the vehicle Jacobian taken between lin and the new pose; lin becomes the new pose."
function predict!(f::FirstEstimates, v::Real, g::Real, wheelbase::Real, Q::AbstractMatrix, dt::Real)
    check(ccall((:slam_ekf_fej_predict, libslamhip_fej), Cint, (Ptr{Cvoid}, Cdouble, Cdouble, Cdouble, Ptr{Cdouble}, Cdouble),
                f.handle, v, g, wheelbase, colmajor4(Q), dt))
    nothing
end

"""
    update!(f, z, R, idf) -> 4 x batches matrix of [v' inv(S) v, log det S, smallest pivot, -1]

The residuals at the current mean, the Jacobians at lin and the first estimates, then the Cholesky-form update.  More than 8
observations go as consecutive batches of 8: the Jacobians do not move between them, the residuals follow the mean.
"""
function update!(f::FirstEstimates, z::AbstractMatrix, R::AbstractMatrix, idf)
    m = size(z, 2)
    ids = Vector{Int32}(vec(collect(idf)))
    length(ids) == m || throw(ArgumentError("idf and z disagree on the number of observations"))
    zz, r = pairs64(z), colmajor4(R)
    outs = zeros(Float64, 4, cld(m, 8))
    for (b, lo) in enumerate(1:8:m)
        hi = min(lo + 7, m)
        out = zeros(Float64, 4)
        check(ccall((:slam_ekf_fej_update, libslamhip_fej), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Int32}, Cint, Ptr{Cdouble}, Ptr{Cdouble}),
                    f.handle, zz[:, lo:hi], ids[lo:hi], hi - lo + 1, r, out))
        outs[:, b] = out
    end
    outs
end

"    augment!(f, z, R): augment! with the new landmarks' Jacobians taken between lin and their new means, which become their first estimates."
function augment!(f::FirstEstimates, z::AbstractMatrix, R::AbstractMatrix)
    size(z, 2) == 0 && return nothing
    check(ccall((:slam_ekf_fej_augment, libslamhip_fej), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Ptr{Cdouble}),
                f.handle, pairs64(z), size(z, 2), colmajor4(R)))
    nothing
end

"    reset!(f; ids = nothing, pose = false): first of the landmarks ids (nothing: all) <- their current means; pose: lin <- the current pose."
function reset!(f::FirstEstimates; ids = nothing, pose::Bool = false)
    sel = ids === nothing ? Int32[] : collect(Int32, ids)
    check(ccall((:slam_ekf_fej_reset, libslamhip_fej), Cint, (Ptr{Cvoid}, Ptr{Int32}, Cint, Cint),
                f.handle, sel, ids === nothing ? -1 : length(sel), pose ? 1 : 0))
    nothing
end

"    remap!(f, ids): after the map was renumbered outside: new landmark j takes the first estimate of old landmark ids[j], 0: its current mean."
function remap!(f::FirstEstimates, ids::AbstractVector{<:Integer})
    sel = collect(Int32, ids)
    check(ccall((:slam_ekf_fej_remap, libslamhip_fej), Cint, (Ptr{Cvoid}, Ptr{Int32}, Cint), f.handle, sel, length(sel)))
    nothing
end

"    transform!(f, tx, ty, theta): lin and every first estimate in another frame; call it beside transform!(s, tx, ty, theta)."
function transform!(f::FirstEstimates, tx::Real, ty::Real, theta::Real)
    check(ccall((:slam_ekf_fej_transform, libslamhip_fej), Cint, (Ptr{Cvoid}, Cdouble, Cdouble, Cdouble), f.handle, tx, ty, theta))
    nothing
end

"    linearisation(f) -> (lin [3], first [2 x count]) as Float64 from the device."
function linearisation(f::FirstEstimates)
    count = Ref{Int32}(0)
    check(ccall((:slam_ekf_fej_get, libslamhip_fej), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Int32}), f.handle, C_NULL, C_NULL, count))
    lin = zeros(Float64, 3); first = zeros(Float64, 2, Int(count[]))
    check(ccall((:slam_ekf_fej_get, libslamhip_fej), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}), f.handle, lin, first, C_NULL))
    lin, first
end

"    set_linearisation!(f, lin, first): write both (first: 2 x N of the state) to the device; the object's count becomes the state's."
function set_linearisation!(f::FirstEstimates, lin::AbstractVector, first::AbstractMatrix)
    check(ccall((:slam_ekf_fej_set, libslamhip_fej), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}),
                f.handle, Vector{Float64}(lin), Matrix{Float64}(first)))
    nothing
end

# ---- the joint update of up to 64 observations (include/ext/slamhip_wide.h; written beside the Python binding, never executed) -----
"    wide_limits() -> observations per joint update call as libslamhip_wide.so reports them."
function wide_limits()
    out = zeros(Int32, 1)
    check(ccall((:slam_ekf_wide_limits, libslamhip_wide), Cint, (Ptr{Int32},), out))
    Int(out[1])
end

# the batches of 64 of update_joint! (commit) and the one call of joint_nis; fh: the FirstEstimates handle, or C_NULL (the stored state)
function wide_batches(commit::Bool, sh::Ptr{Cvoid}, fh::Ptr{Cvoid}, z::AbstractMatrix, R::AbstractMatrix, idf)
    m = size(z, 2)
    ids = Vector{Int32}(vec(collect(idf)))
    length(ids) == m || throw(ArgumentError("idf and z disagree on the number of observations"))
    zz, r = pairs64(z), colmajor4(R)
    outs = zeros(Float64, 4, cld(m, 64))
    for (b, lo) in enumerate(1:64:m)
        hi = min(lo + 63, m)
        out = zeros(Float64, 4)
        if commit
            check(ccall((:slam_ekf_wide_update, libslamhip_wide), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Int32}, Cint, Ptr{Cdouble}, Ptr{Cdouble}),
                        sh, fh, zz[:, lo:hi], ids[lo:hi], hi - lo + 1, r, out))
        else
            check(ccall((:slam_ekf_wide_nis, libslamhip_wide), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Int32}, Cint, Ptr{Cdouble}, Ptr{Cdouble}),
                        sh, fh, zz[:, lo:hi], ids[lo:hi], hi - lo + 1, r, out))
        end
        outs[:, b] = out
    end
    outs
end

"""
    update_joint!(f, z, R, idf) -> 4 x batches matrix of [v' inv(S) v, log det S, smallest pivot, -1]

`update!(f, ...)` of up to 64 observations JOINTLY, in one pass over the covariance: every residual at the mean before the call, every
Jacobian at lin and the first estimates.  More than 64 go as consecutive batches of 64.  `update_joint!(s, z, R, idf)` on a state
takes the Jacobians at the stored state: the Cholesky-form `ekf_update!` by the wide front half.
"""
update_joint!(f::FirstEstimates, z::AbstractMatrix, R::AbstractMatrix, idf) = wide_batches(true, handle(f.state), f.handle, z, R, idf)
update_joint!(s::EKFSlamState, z::AbstractMatrix, R::AbstractMatrix, idf) = wide_batches(true, handle(s), C_NULL, z, R, idf)

"    joint_nis(f, z, R, idf) -> what update_joint! would return for at most 64 observations, the state only read."
function joint_nis(f::FirstEstimates, z::AbstractMatrix, R::AbstractMatrix, idf)
    size(z, 2) <= 64 || throw(ArgumentError("joint_nis takes at most 64 observations"))
    wide_batches(false, handle(f.state), f.handle, z, R, idf)
end

# ---- compressed local-area updates (include/ext/slamhip_local.h) -----------------------------------------------------------------
"""
    LocalArea(s, ids; max_local = min(1024, length(ids) + 64))

The compressed EKF over the vehicle and the landmarks `ids` of `s` (local landmark j is ids[j]; landmarks added in the area
follow): `ekf_predict!`, `ekf_update!` (local ids, Cholesky form), `augment!`, `associate` and `observe!` work on a small state,
`close!` brings `s` up to date in one pass (up to rounding the full filter's result), `abort!` discards the area.  While the area
is open `s` must not be written.  `open_area!(a, ids)` opens the next area on the same object.
"""
mutable struct LocalArea{T<:Union{Float32,Float64}}
    handle::Ptr{Cvoid}
    parent::EKFSlamState{T}
    state::Ptr{Cvoid}                             # the local EKF handle, owned by the library
    ids::Vector{Int32}
    function LocalArea(s::EKFSlamState{T}, ids::AbstractVector{<:Integer} = Int32[];
                       max_local::Integer = min(1024, max(1, length(ids) + 64)), open::Bool = true) where {T}
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:slam_ekf_local_create, libslamhip_local), Cint, (Ref{Ptr{Cvoid}}, Ptr{Cvoid}, Cint), h, handle(s), max_local))
        l = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:slam_ekf_local_state, libslamhip_local), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), h[], l))
        a = new{T}(h[], s, l[], Int32[])
        finalizer(a) do ar
            ccall((:slam_ekf_local_destroy, libslamhip_local), Cint, (Ptr{Cvoid},), ar.handle)
        end
        open && open_area!(a, ids)
        return a
    end
end

function open_area!(a::LocalArea, ids::AbstractVector{<:Integer})
    sel = collect(Int32, ids)
    check(ccall((:slam_ekf_local_open, libslamhip_local), Cint, (Ptr{Cvoid}, Ptr{Int32}, Cint), a.handle, sel, length(sel)))
    a.ids = sel
    a
end

"    close!(a) -> first_new: the global state is brought up to date; the landmarks added in the area are first_new, first_new + 1, ..."
function close!(a::LocalArea)
    first = Ref{Cint}(0)
    check(ccall((:slam_ekf_local_close, libslamhip_local), Cint, (Ptr{Cvoid}, Ref{Cint}), a.handle, first))
    Int(first[])
end

"    abort!(a): discard the area; the global state is untouched."
abort!(a::LocalArea) = (check(ccall((:slam_ekf_local_abort, libslamhip_local), Cint, (Ptr{Cvoid},), a.handle)); nothing)

"    area_info(a) -> (open, n0, n_a, added, steps, N_open, max_local)"
function area_info(a::LocalArea)
    out = zeros(Int64, 8)
    check(ccall((:slam_ekf_local_info, libslamhip_local), Cint, (Ptr{Cvoid}, Ptr{Int64}), a.handle, out))
    (open = out[1] != 0, n0 = Int(out[2]), n_a = Int(out[3]), added = Int(out[4]), steps = Int(out[5]), N_open = Int(out[6]),
     max_local = Int(out[7]))
end

"    global_ids(a): the global id of every local landmark, in local order."
function global_ids(a::LocalArea)
    i = area_info(a)
    vcat(a.ids, Int32.(i.N_open .+ (1:i.added)))
end

"    accumulators(a) -> (phi n_a x n0, psi n0 x n0, theta n0), Float64 (the library returns row-major: transposed here)."
function accumulators(a::LocalArea)
    i = area_info(a)
    phi = Matrix{Float64}(undef, i.n0, i.n_a); psi = Matrix{Float64}(undef, i.n0, i.n0); theta = Vector{Float64}(undef, i.n0)
    check(ccall((:slam_ekf_local_get, libslamhip_local), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                a.handle, phi, psi, theta))
    permutedims(phi), permutedims(psi), theta
end

"    local_state(a) -> (x, P) of the local state."
function local_state(a::LocalArea{T}) where {T}
    n = area_info(a).n_a
    x = Vector{T}(undef, n); P = Matrix{T}(undef, n, n)
    check(ccall((:slam_ekf_get_state, libslamhip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint), a.state, x, P, n, n))
    x, P
end

function ekf_predict!(a::LocalArea, v::Real, g::Real, wheelbase::Real, Q::AbstractMatrix, dt::Real)
    check(ccall((:slam_ekf_local_predict, libslamhip_local), Cint, (Ptr{Cvoid}, Cdouble, Cdouble, Cdouble, Ptr{Cdouble}, Cdouble),
                a.handle, v, g, wheelbase, colmajor4(Q), dt))
    nothing
end

function ekf_update!(a::LocalArea, z::AbstractMatrix, R::AbstractMatrix, idf; form::Symbol = :cholesky)
    ids = collect(Int32, vec(collect(idf)))
    check(ccall((:slam_ekf_local_update, libslamhip_local), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Int32}, Cint, Ptr{Cdouble}, Cint),
                a.handle, pairs64(z), ids, length(ids), colmajor4(R), form === :joseph ? FORM_JOSEPH : FORM_CHOLESKY))
    nothing
end

function augment!(a::LocalArea, z::AbstractMatrix, R::AbstractMatrix)
    size(z, 2) == 0 && return nothing
    check(ccall((:slam_ekf_local_augment, libslamhip_local), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Ptr{Cdouble}),
                a.handle, pairs64(z), size(z, 2), colmajor4(R)))
    nothing
end

"associate(a, z, R, gate1, gate2) -> (zf, idf, zn) against the LOCAL map: idf are local ids."
function associate(a::LocalArea, z::AbstractMatrix, R::AbstractMatrix, gate1::Real, gate2::Real)
    nz = size(z, 2)
    assoc = zeros(Int32, nz)
    if nz > 0
        check(ccall((:slam_ekf_associate, libslamhip), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cdouble, Cdouble, Ptr{Int32}),
                    a.state, pairs64(z), nz, colmajor4(R), gate1, gate2, assoc))
    end
    hit = findall(>(0), assoc)
    z[:, hit], reshape(Int.(assoc[hit]), 1, :), z[:, findall(<(0), assoc)]
end

"observe!(a, z, R, gate1, gate2): associate on the local state, then update, then augment; returns (zf, idf, zn)."
function observe!(a::LocalArea, z::AbstractMatrix, R::AbstractMatrix, gate1::Real, gate2::Real)
    zf, idf, zn = associate(a, z, R, gate1, gate2)
    size(zf, 2) > 0 && ekf_update!(a, zf, R, idf)
    augment!(a, zn, R)
    zf, idf, zn
end

"    landmarks_within(s, cx, cy, r): the ids of the landmarks whose mean lies within r of (cx, cy), from the downloaded mean."
function landmarks_within(s::EKFSlamState, cx::Real, cy::Real, r::Real)
    x = download(s, :x)
    Int32[j for j in 1:nlandmarks(s) if hypot(x[2 + 2j] - cx, x[3 + 2j] - cy) <= r]
end

"feature_ellipses(x, cov) of the browser monitor (sim/browser/wsserver.jl:72-85): 5 x N [cx; cy; rx; ry; phi], on the device."
function feature_ellipses(s::EKFSlamState)
    out = Matrix{Float64}(undef, 5, nlandmarks(s))
    check(ccall((:slam_ekf_ellipses, libslamhip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), handle(s), out, C_NULL))
    out
end

"The vehicle-ellipse record of monitor() (sim/browser/wsserver.jl:60-65): [cx, cy, vehicle_phi, rx, ry, phi]."
function vehicle_ellipse(s::EKFSlamState)
    out = zeros(Float64, 6)
    check(ccall((:slam_ekf_ellipses, libslamhip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), handle(s), C_NULL, out))
    out
end

# ---- the reference's function surface ------------------------------------------------------
# The reference returns (x, P) and its only caller assigns them back to the state
# (sim/ekfslam-sim.jl:100,117,120).  Here the state was already updated in place, so the
# returned pair is (nothing, nothing) and `setproperty!` ignores it -- no 1.6 GB round trip.

"predict(state, vehicle, Q, dt): `vehicle` needs measured_speed, measured_gamma, wheelbase (src/ekf.jl:14-16)."
function predict(s::EKFSlamState, vehicle, Q::AbstractMatrix, dt::AbstractFloat)
    ekf_predict!(s, vehicle.measured_speed, vehicle.measured_gamma, vehicle.wheelbase, Q, dt)
    nothing, nothing
end

function update(s::EKFSlamState, z, R, idf)
    ekf_update!(s, z, R, idf)
    nothing, nothing
end

function add_features(s::EKFSlamState, z, R)
    augment!(s, z, R)
    nothing, nothing
end

"associate(state, z, R, gate1, gate2) -> (zf 2 x nf, idf 1 x nf Int, zn 2 x nn)  (src/data-association.jl:1-51)."
function associate(s::EKFSlamState, z::AbstractMatrix, R::AbstractMatrix, gate1::Real, gate2::Real)
    nz = size(z, 2)
    assoc = zeros(Int32, nz)
    if nz > 0
        check(ccall((:slam_ekf_associate, libslamhip), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cdouble, Cdouble, Ptr{Int32}),
                    handle(s), pairs64(z), nz, colmajor4(R), gate1, gate2, assoc))
    end
    hit = findall(>(0), assoc)
    new = findall(<(0), assoc)
    z[:, hit], reshape(Int.(assoc[hit]), 1, :), z[:, new]
end

# ---- joint-compatibility data association (include/slamhip_jc.h; no counterpart in the reference) -------------------------------
"""
    chi2_table(m, confidence = 0.95)

Thresholds of the joint-compatibility search: entry k is the chi-square quantile at `confidence` with 2k degrees of freedom, from the
closed form for even degrees of freedom, 1 - exp(-x/2) sum_{i<k} (x/2)^i / i!, by bisection.
"""
function chi2_table(m::Integer, confidence::Real = 0.95)
    0 < confidence < 1 || error("confidence must lie strictly between 0 and 1")
    function cdf(x, k)
        h, term, acc = x / 2, 1.0, 0.0
        for i in 0:k-1
            acc += term
            term *= h / (i + 1)
        end
        1 - exp(-h) * acc
    end
    out = zeros(Float64, m)
    for k in 1:m
        lo, hi = 0.0, 4.0 * k + 16.0
        while cdf(hi, k) < confidence
            hi *= 2
        end
        for _ in 1:200
            mid = (lo + hi) / 2
            (mid == lo || mid == hi) && break
            cdf(mid, k) < confidence ? (lo = mid) : (hi = mid)
        end
        out[k] = (lo + hi) / 2
    end
    out
end

function jc_handle(s::EKFSlamState)
    if getfield(s, :jc) == C_NULL
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:slam_ekf_jc_create, libslamhip_jc), Cint, (Ref{Ptr{Cvoid}}, Ptr{Cvoid}), h, handle(s)))
        setfield!(s, :jc, h[])
    end
    getfield(s, :jc)
end

"The association vector (j >= 1 matched, 0 dropped, -1 new) and the info record of slam_ekf_associate_joint."
function associate_joint_vector(s::EKFSlamState, z::AbstractMatrix, R::AbstractMatrix, gate1::Real, gate2::Real;
                                confidence::Real = 0.95, max_nodes::Integer = 20000)
    nz = size(z, 2)
    assoc = zeros(Int32, nz)
    info = zeros(Float64, 8)
    chi2 = chi2_table(max(nz, 1), confidence)
    check(ccall((:slam_ekf_associate_joint, libslamhip_jc), Cint,
                (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cdouble, Cdouble, Ptr{Cdouble}, Int64, Ptr{Int32}, Ptr{Cdouble}),
                jc_handle(s), pairs64(z), nz, colmajor4(R), gate1, gate2, chi2, max_nodes, assoc, info))
    assoc, (pairings = Int(info[1]), d2 = info[2], tests = Int(info[3]), exhausted = info[4] != 0, truncated = info[5] != 0,
            candidates = Int(info[6]), deepest = Int(info[7]))
end

"""
    associate_joint(state, z, R, gate1, gate2; confidence = 0.95, max_nodes = 20000) -> (zf, idf, zn, info)

`associate` with the decisions of the joint-compatibility search: the largest set of pairings, each landmark used at most once, whose
stacked innovation passes the chi-square test against the joint innovation covariance (at most 64 observations).  The state is not
changed.
"""
function associate_joint(s::EKFSlamState, z::AbstractMatrix, R::AbstractMatrix, gate1::Real, gate2::Real; kw...)
    assoc, info = associate_joint_vector(s, z, R, gate1, gate2; kw...)
    hit = findall(>(0), assoc)
    new = findall(<(0), assoc)
    z[:, hit], reshape(Int.(assoc[hit]), 1, :), z[:, new], info
end

"associate_joint, then ekf_update!, then augment!  -> (association vector, info)."
function observe_joint!(s::EKFSlamState, z::AbstractMatrix, R::AbstractMatrix, gate1::Real, gate2::Real;
                        form::Symbol = :cholesky, kw...)
    assoc, info = associate_joint_vector(s, z, R, gate1, gate2; kw...)
    hit = findall(>(0), assoc)
    new = findall(<(0), assoc)
    isempty(hit) || ekf_update!(s, z[:, hit], R, Int.(assoc[hit]); form = form)
    isempty(new) || augment!(s, z[:, new], R)
    assoc, info
end

"d2 = v' inv(S_H) v of the hypothesis observation i <-> landmark idf[i] (1-based, distinct) under the joint covariance (slam_ekf_joint_nis)."
function joint_nis(s::EKFSlamState, z::AbstractMatrix, idf, R::AbstractMatrix)
    ids = Int32.(vec(collect(idf)))
    length(ids) == size(z, 2) || error("idf and z disagree on the number of observations")
    out = Ref{Cdouble}(0.0)
    check(ccall((:slam_ekf_joint_nis, libslamhip_jc), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Int32}, Cint, Ptr{Cdouble}, Ref{Cdouble}),
                jc_handle(s), pairs64(z), ids, length(ids), colmajor4(R), out))
    out[]
end

"compute_association(state, z, R, idf) -> (nis, nd)  (src/data-association.jl:53-63; x, P are the state's)."
function compute_association(s::EKFSlamState, z::AbstractVector, R::AbstractMatrix, idf::Integer)
    out = zeros(Float64, 2)
    check(ccall((:slam_ekf_nis, libslamhip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}),
                handle(s), Float64[z[1], z[2]], idf, colmajor4(R), out))
    out[1], out[2]
end

"predict_observation(state, idf) -> (z, H) with H dense 2 x n (src/common.jl:139-165)."
function predict_observation(s::EKFSlamState, idf::Integer)
    zp = zeros(2); Hv = zeros(2, 3); Hf = zeros(2, 2)
    check(ccall((:slam_ekf_predict_observation, libslamhip), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}), handle(s), idf, zp, Hv, Hf))
    H = zeros(2, length(s))
    H[:, 1:3] = Hv
    fpos = 3 + 2 * idf - 1
    H[:, fpos:fpos+1] = Hf
    zp, H
end

# ---- PFSlamState: the FastSLAM-1.0 particle filter -----------------------------------------------
# The reference declares `Particle` / `PFSlamState` (src/common.jl:14-20,31-34) and no filter code (README.md:6);
# the algorithm is the one specified from the reference's EKF building blocks (include/slamhip.h, "FastSLAM").
# Every call is one `ccall`.  A filter SHARDED over several GPUs (one Julia process per GPU, or one task per GPU in
# one process) needs no collective library either: each rank constructs its slice (`rank`, `world`), the ranks swap
# their `peer_blob`s once (MPI.Allgather, a shared file, Distributed -- 1 KB per rank) and `attach_peers!`; from then on
# the per-step scalars travel GPU to GPU and a resampling step stays on the device (include/slamhip.h, "peers").

const SLAM_PF_PEER_BLOB_BYTES = 4096

"""
    PFSlamState{T}(n, max_landmarks; seed = 0, device = 0, rank = 0, world = 1)

`PFSlamState{T}` (src/common.jl:31-34) with `n` particles IN ALL, device resident (structure of arrays:
`pose[3][n]`, `logw[n]`, `lm[max_landmarks][5][n]`).  `world > 1`: this process owns the global particle ids
`rank * n / world ... (rank + 1) * n / world - 1` on its GPU; see `peer_blob` / `attach_peers!`.
"""
mutable struct PFSlamState{T<:Union{Float32,Float64}} <: SlamState
    handle::Ptr{Cvoid}
    n::Int                  # particles on THIS rank
    max_landmarks::Int
    rank::Int
    world::Int
    function PFSlamState{T}(n::Integer, max_landmarks::Integer; seed::Integer = 0, device::Integer = 0, rank::Integer = 0,
                            world::Integer = 1) where {T}
        n % world == 0 || error("n must be divisible by the number of ranks")
        per = div(n, world)
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:slam_pf_create, libslamhip), Cint,
                    (Ref{Ptr{Cvoid}}, Cint, Int64, Int64, Int64, Cint, Cint, UInt64),
                    h, T === Float32 ? SLAM_F32 : SLAM_F64, per, n, rank * per, max_landmarks, device, seed))
        s = new{T}(h[], per, max_landmarks, rank, world)
        finalizer(s) do st
            ccall((:slam_pf_destroy, libslamhip), Cint, (Ptr{Cvoid},), st.handle)
        end
        return s
    end
end

"This rank's peer blob (IPC handles of its buffers and inbox): every rank needs every rank's."
function peer_blob(s::PFSlamState)
    blob = zeros(UInt8, SLAM_PF_PEER_BLOB_BYTES)
    check(ccall((:slam_pf_export_peer, libslamhip), Cint, (Ptr{Cvoid}, Ptr{UInt8}), s.handle, blob))
    blob
end

"`blobs`: the `world` peer blobs in rank order.  Afterwards `step_async!` resamples the sharded filter on the device."
function attach_peers!(s::PFSlamState, blobs::AbstractVector)
    length(blobs) == s.world || error("one blob per rank")
    all = reduce(vcat, [Vector{UInt8}(b) for b in blobs])
    check(ccall((:slam_pf_attach_peers, libslamhip), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{UInt8}), s.handle, s.rank, s.world, all))
    s
end

"Collective: true when every attached peer's inbox write arrived within `timeout_ms` (call right after `attach_peers!`)."
function peer_selftest(s::PFSlamState, timeout_ms::Integer = 3000)
    ccall((:slam_pf_peer_selftest, libslamhip), Cint, (Ptr{Cvoid}, Cint), s.handle, timeout_ms) == 0
end

"Collective: remote records come home, the peers are detached (call on every rank before any rank lets its state go)."
function detach_peers!(s::PFSlamState)
    check(ccall((:slam_pf_detach_peers, libslamhip), Cint, (Ptr{Cvoid},), s.handle))
    s
end

"[ranks, 1 if peers are attached, SLAM_PF_HALTED returns so far, resamplings so far]"
function comm_info(s::PFSlamState)
    out = zeros(Int64, 4)
    check(ccall((:slam_pf_comm_info, libslamhip), Cint, (Ptr{Cvoid}, Ptr{Int64}), s.handle, out))
    out
end

"Every particle at `pose`, uniform weights (Particle.pose, src/common.jl:15)."
function set_pose!(s::PFSlamState, pose::AbstractVector)
    check(ccall((:slam_pf_set_pose, libslamhip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), s.handle, Float64[pose[1], pose[2], pose[3]]))
    s
end

"Landmarks 1..size(xy, 2) known to every particle at xy (2 x nl) + N(0, jitter^2), covariance diag(var, var)."
function init_landmarks!(s::PFSlamState, xy::AbstractMatrix, var::Real, jitter::Real)
    check(ccall((:slam_pf_init_landmarks, libslamhip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cdouble, Cdouble),
                s.handle, Matrix{Float64}(xy), size(xy, 2), var, jitter))
    s
end

"F1: control noise per particle (sim/sim-utils.jl:35-38) + the pose update of predict (src/ekf.jl:39-41)."
function pf_predict!(s::PFSlamState, V::Real, G::Real, wheelbase::Real, Q::AbstractMatrix, dt::Real)
    check(ccall((:slam_pf_predict, libslamhip), Cint, (Ptr{Cvoid}, Cdouble, Cdouble, Cdouble, Ptr{Cdouble}, Cdouble),
                s.handle, V, G, wheelbase, colmajor4(Q), dt))
    s
end

"F2/F3: z (2 x m) with known 1-based landmark ids; per-landmark 2 x 2 EKF update, log-weights, first sightings."
function update_known!(s::PFSlamState, z::AbstractMatrix, ids, R::AbstractMatrix)
    m = size(z, 2)
    m == 0 && return s
    check(ccall((:slam_pf_update_known, libslamhip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Int32}, Cint, Ptr{Cdouble}),
                s.handle, pairs64(z), Vector{Int32}(vec(collect(ids))), m, colmajor4(R)))
    s
end

"""
    step_unknown!(state, V, G, wheelbase, Q, dt, z, R, gate1, gate2) -> [max logw, sum, sum2]

Predict, per-particle association of the (range, bearing) pairs `z` (2 x m, m <= 64, UNKNOWN correspondences) against each
particle's own landmarks, updates / new landmarks and the local weight statistics as one sweep (slam_pf_step_unknown).
"""
function step_unknown!(s::PFSlamState, V::Real, G::Real, wheelbase::Real, Q::AbstractMatrix, dt::Real, z::AbstractMatrix,
                       R::AbstractMatrix, gate1::Real, gate2::Real)
    out = zeros(Float64, 3)
    check(ccall((:slam_pf_step_unknown, libslamhip), Cint,
                (Ptr{Cvoid}, Cdouble, Cdouble, Cdouble, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cdouble, Cdouble,
                 Ptr{Int32}, Ptr{Cdouble}),
                s.handle, V, G, wheelbase, colmajor4(Q), dt, pairs64(z), size(z, 2), colmajor4(R), gate1, gate2,
                Ptr{Int32}(C_NULL), out))
    out
end

"""
    step_proposal_unknown!(state, V, G, wheelbase, Q, dt, z, R, gate1, gate2; d_assoc = C_NULL) -> [max logw, sum, sum2]

FastSLAM 2.0 with UNKNOWN correspondences (slam_pf_step_proposal_unknown, include/ext/slamhip_proposal.h): every particle
associates the (range, bearing) pairs `z` (2 x m, m <= proposal_max_obs()) with its own landmarks under the prior proposal, draws
its pose from the proposal that knows the matched ones and updates its map from the sampled pose.  `Q` is any symmetric positive
definite 2 x 2 matrix.  `d_assoc`: a DEVICE array ([m][n] Int32) that receives the decisions (slot >= 0, -1 new, -2 dropped).
Whole filter on one shard; the call synchronises.
"""
function step_proposal_unknown!(s::PFSlamState, V::Real, G::Real, wheelbase::Real, Q::AbstractMatrix, dt::Real, z::AbstractMatrix,
                                R::AbstractMatrix, gate1::Real, gate2::Real; d_assoc::Ptr{Int32} = Ptr{Int32}(C_NULL))
    out = zeros(Float64, 3)
    check(ccall((:slam_pf_step_proposal_unknown, libslamhip_proposal), Cint,
                (Ptr{Cvoid}, Cdouble, Cdouble, Cdouble, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cdouble, Cdouble,
                 Ptr{Int32}, Ptr{Cdouble}),
                s.handle, V, G, wheelbase, colmajor4(Q), dt, pairs64(z), size(z, 2), colmajor4(R), gate1, gate2, d_assoc, out))
    out
end

"""
    associate_proposal(state, V, G, wheelbase, Q, dt, z, R, gate1, gate2, d_assoc; d_nis = C_NULL)

The association of `step_proposal_unknown!` alone (slam_pf_associate_proposal): the state is only read.  `d_assoc` ([m][n] Int32)
and `d_nis` ([m][n] in the state's element type: the nis of the winning slot, NaN where nothing matched) are DEVICE arrays; the
call is enqueued on the filter's stream.
"""
function associate_proposal(s::PFSlamState, V::Real, G::Real, wheelbase::Real, Q::AbstractMatrix, dt::Real, z::AbstractMatrix,
                            R::AbstractMatrix, gate1::Real, gate2::Real, d_assoc::Ptr{Int32}; d_nis::Ptr{Cvoid} = C_NULL)
    check(ccall((:slam_pf_associate_proposal, libslamhip_proposal), Cint,
                (Ptr{Cvoid}, Cdouble, Cdouble, Cdouble, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cdouble, Cdouble,
                 Ptr{Int32}, Ptr{Cvoid}),
                s.handle, V, G, wheelbase, colmajor4(Q), dt, pairs64(z), size(z, 2), colmajor4(R), gate1, gate2, d_assoc, d_nis))
    s
end

"Observations per call of `step_proposal_unknown!`, as the library reports it (slam_pf_proposal_limits)."
function proposal_max_obs()
    out = zeros(Cint, 4)
    check(ccall((:slam_pf_proposal_limits, libslamhip_proposal), Cint, (Ptr{Cint},), out))
    Int(out[1])
end

"""
    LandmarkEvidence(state, r_max, half_fov; inc = 1, dec = 1, init = 1, cap = 5)

Landmark evidence of an unknown-correspondence filter (include/slamhip_evidence.h): one Int8 existence counter per (slot,
particle) on the device, raised by `inc` (up to `cap`) when the step matched the slot, lowered by `dec` when the landmark lies
within `r_max` and +-`half_fov` of the particle's pose and was not observed; below zero the record is discarded.  Only a filter
that lives wholly on one rank (`world == 1`).  The object borrows `state` (kept alive through the field) and must be the only
way the filter is resampled: `step_unknown_pruned!` does that.
"""
mutable struct LandmarkEvidence
    handle::Ptr{Cvoid}
    state::PFSlamState
    r_max::Float64
    half_fov::Float64
    inc::Int
    dec::Int
    init::Int
    cap::Int
    resamples::Int
    function LandmarkEvidence(s::PFSlamState, r_max::Real, half_fov::Real; inc::Integer = 1, dec::Integer = 1, init::Integer = 1,
                              cap::Integer = 5)
        s.world == 1 || error("landmark evidence supports only a filter that lives wholly on one rank")
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:slam_pf_evidence_create, libslamhip_evidence), Cint, (Ref{Ptr{Cvoid}}, Ptr{Cvoid}), h, s.handle))
        e = new(h[], s, r_max, half_fov, inc, dec, init, cap, 0)
        finalizer(e) do ev
            ccall((:slam_pf_evidence_destroy, libslamhip_evidence), Cint, (Ptr{Cvoid},), ev.handle)
        end
        return e
    end
end

"One pass of the rule with the DEVICE array `d_assoc` ([m][n] Int32) of the step just made: [in use, created, decremented, pruned]."
function evidence_update!(e::LandmarkEvidence, d_assoc::Ptr{Int32}, m::Integer)
    counts = zeros(Int64, 4)
    check(ccall((:slam_pf_evidence_update, libslamhip_evidence), Cint,
                (Ptr{Cvoid}, Ptr{Int32}, Cint, Cdouble, Cdouble, Cint, Cint, Cint, Cint, Ptr{Int64}),
                e.handle, d_assoc, m, e.r_max, e.half_fov, e.inc, e.dec, e.init, e.cap, counts))
    counts
end

"The counters, `max_landmarks x n` Int8 (-128: no landmark in that slot of that particle)."
function counters(e::LandmarkEvidence)
    out = zeros(Int8, e.state.n, e.state.max_landmarks)          # the library's [nl][n], particle index fastest
    check(ccall((:slam_pf_evidence_get, libslamhip_evidence), Cint, (Ptr{Cvoid}, Ptr{Int8}), e.handle, out))
    permutedims(out)
end

# One U(0,1) from Philox4x32-10 with counter (0, 0, step, stream): the systematic-resampling offset (pf.py: philox_uniform)
function philox_uniform(step::Integer, stream::Integer, seed::Integer)
    c = UInt32[0, 0, step % UInt32, stream % UInt32]
    k0, k1 = UInt32(seed & 0xffffffff), UInt32((seed >> 32) & 0xffffffff)
    for _ in 1:10
        p0, p1 = UInt64(0xD2511F53) * c[1], UInt64(0xCD9E8D57) * c[3]
        c = UInt32[(p1 >> 32) % UInt32 ⊻ c[2] ⊻ k0, p1 % UInt32, (p0 >> 32) % UInt32 ⊻ c[4] ⊻ k1, p0 % UInt32]
        k0 += 0x9E3779B9
        k1 += 0xBB67AE85
    end
    ((c[1] >> 8) + 0.5) / 16777216.0
end

"""
    step_unknown_pruned!(state, evidence, V, G, wheelbase, Q, dt, z, R, gate1, gate2; neff_frac = 0.75, seed = 0)
        -> (Neff, resampled, counts)

`step_unknown!` with landmark evidence (slam_pf_step_unknown_evidence), the normalisation, and -- if Neff < neff_frac * n --
systematic resampling through slam_pf_evidence_resample, so that the counters follow their particles.  `seed`: the filter's seed
(it keys the resampling offset).  `counts` = [records in use, created, decremented, pruned] of this step.
"""
function step_unknown_pruned!(s::PFSlamState{T}, e::LandmarkEvidence, V::Real, G::Real, wheelbase::Real, Q::AbstractMatrix, dt::Real,
                              z::AbstractMatrix, R::AbstractMatrix, gate1::Real, gate2::Real; neff_frac::Real = 0.75,
                              seed::Integer = 0) where {T}
    e.state === s || error("the evidence object belongs to another filter")
    out = zeros(Float64, 3)
    counts = zeros(Int64, 4)
    check(ccall((:slam_pf_step_unknown_evidence, libslamhip_evidence), Cint,
                (Ptr{Cvoid}, Cdouble, Cdouble, Cdouble, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cdouble, Cdouble,
                 Cdouble, Cdouble, Cint, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Int64}),
                e.handle, V, G, wheelbase, colmajor4(Q), dt, pairs64(z), size(z, 2), colmajor4(R), gate1, gate2,
                e.r_max, e.half_fov, e.inc, e.dec, e.init, e.cap, out, counts))
    gmax, s1, s2 = out
    check(ccall((:slam_pf_normalize, libslamhip), Cint, (Ptr{Cvoid}, Cdouble, Cdouble), s.handle, gmax, s1))
    neff = s1 * s1 / s2
    did = neff < neff_frac * s.n
    if did
        gnorm = Float64(T(gmax) - T(gmax + log(s1)))      # the largest log-weight after the shift, as stored
        check(ccall((:slam_pf_evidence_resample, libslamhip_evidence), Cint, (Ptr{Cvoid}, Cdouble, Cdouble),
                    e.handle, gnorm, philox_uniform(e.resamples, 2, seed)))
        e.resamples += 1
        check(ccall((:slam_pf_set_resample_count, libslamhip), Cint, (Ptr{Cvoid}, Int64), s.handle, e.resamples))
    end
    neff, did, counts
end

"""
    transform!(state, tx, ty, theta) -> state

Express the filter in another frame (slam_pf_transform): every particle's pose and every landmark record in use through
p <- R(theta) p + (tx, ty), Pf <- R Pf R'; the log-weights and the RNG step are untouched.  Enqueued.
"""
function transform!(s::PFSlamState, tx::Real, ty::Real, theta::Real)
    check(ccall((:slam_pf_transform, libslamhip_frame), Cint, (Ptr{Cvoid}, Cdouble, Cdouble, Cdouble), s.handle, tx, ty, theta))
    s
end

"""
    step!(state, V, G, wheelbase, Q, dt, z, ids, R; neff_frac = 0.75, proposal = false) -> (Neff, resampled)

One whole filter step, synchronously: predict (or the FastSLAM-2.0 proposal), the known-id updates, the weights, the
normalisation, and systematic resampling if Neff < neff_frac * n.
"""
function step!(s::PFSlamState, V::Real, G::Real, wheelbase::Real, Q::AbstractMatrix, dt::Real, z::AbstractMatrix, ids,
               R::AbstractMatrix; neff_frac::Real = 0.75, proposal::Bool = false)
    step_async!(s, V, G, wheelbase, Q, dt, z, ids, R; neff_frac = neff_frac, proposal = proposal)
    out = flush!(s)
    out[1], out[2] != 0
end

"The same step ENQUEUED (slam_pf_step_auto): Neff, the decision and the resampling stay on the device; `flush!` waits."
function step_async!(s::PFSlamState, V::Real, G::Real, wheelbase::Real, Q::AbstractMatrix, dt::Real, z::AbstractMatrix, ids,
                     R::AbstractMatrix; neff_frac::Real = 0.75, force::Integer = -1, proposal::Bool = false)
    check(ccall((:slam_pf_step_auto, libslamhip), Cint,
                (Ptr{Cvoid}, Cdouble, Cdouble, Cdouble, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Int32}, Cint, Ptr{Cdouble},
                 Cdouble, Cint, Cint),
                s.handle, V, G, wheelbase, colmajor4(Q), dt, pairs64(z), Vector{Int32}(vec(collect(ids))), size(z, 2),
                colmajor4(R), neff_frac, force, proposal ? 1 : 0))
    s
end

"""
K `step_async!` calls as ONE (slam_pf_step_auto_batch): `controls` is K x 2 (V, G per row), `obs` a vector of K pairs `(z, ids)`
(z 2 x m_k), `force` a vector of K integers (-1 the Neff rule, 0 never, 1 always).  Runs of at least four consecutive steps that
cannot resample go as one persistent launch where the filter allows it and `persistent = true` says that nothing else keeps the
device busy meanwhile; the result is the K calls' bit for bit.
"""
function step_async_batch!(s::PFSlamState, controls::AbstractMatrix, wheelbase::Real, Q::AbstractMatrix, dt::Real, obs::AbstractVector,
                           R::AbstractMatrix; neff_frac::Real = 0.75, force::AbstractVector = fill(-1, length(obs)),
                           proposal::Bool = false, persistent::Bool = false)
    K = length(obs)
    ms = Int32[size(o[1], 2) for o in obs]
    stride = max(1, maximum(ms; init = 0))
    zz = zeros(Float64, 2, stride, K)                 # (range, bearing) pairs, zstride pairs per step
    ii = zeros(Int32, stride, K)
    for k in 1:K
        zz[:, 1:ms[k], k] = obs[k][1]
        ii[1:ms[k], k] = vec(collect(obs[k][2]))
    end
    vg = Matrix{Float64}(transpose(Float64.(controls)))      # 2 x K: (V, G) per step, contiguous
    took = Ref{Cint}(0)
    check(ccall((:slam_pf_step_auto_batch, libslamhip), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Int32}, Ptr{Int32}, Cint, Ptr{Cdouble},
                 Cdouble, Ptr{Int32}, Cint, Cint, Ref{Cint}),
                s.handle, K, vg, wheelbase, colmajor4(Q), dt, zz, ii, ms, stride, colmajor4(R), neff_frac,
                Vector{Int32}(force), proposal ? 1 : 0, persistent ? 2 : 0, took))
    s
end

"Wait for the queued steps: [Neff of the last step, 1.0 if it resampled, resamplings so far, steps so far]."
function flush!(s::PFSlamState)
    out = zeros(Float64, 4)
    check(ccall((:slam_pf_flush, libslamhip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), s.handle, out))
    out
end

"F4: normalise, and resample if Neff < neff_frac * n.  Returns whether it resampled."
function resample!(s::PFSlamState, neff_frac::Real = 0.75)
    did = Ref{Cint}(0)
    check(ccall((:slam_pf_resample, libslamhip), Cint, (Ptr{Cvoid}, Cdouble, Ref{Cint}), s.handle, neff_frac, did))
    did[] != 0
end

"Weighted mean pose [x, y, phi]."
function mean_pose(s::PFSlamState)
    out = zeros(Float64, 3)
    check(ccall((:slam_pf_get_mean_pose, libslamhip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), s.handle, out))
    out
end

"The particles' weights (Particle.weight, src/common.jl:19)."
function weights(s::PFSlamState)
    out = zeros(Float64, s.n)
    check(ccall((:slam_pf_get_weights, libslamhip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), s.handle, out))
    out
end

"""
The map of the filter (whole filter on this shard) without downloading the particles: 8 x cnt matrix, per landmark
[mass, mean x, mean y, Cxx, Cxy, Cyy, count, 0] -- the moment-matched Gaussian of the particles' mixture
(slam_pf_get_map).  `ids`: 1-based landmark ids, `nothing` = all.
"""
function pf_map(s::PFSlamState, ids::Union{Nothing,AbstractVector} = nothing)
    cnt = ids === nothing ? s.max_landmarks : length(ids)
    out = zeros(Float64, 8, cnt)
    idv = ids === nothing ? Ptr{Int32}(C_NULL) : Vector{Int32}(ids)
    check(ccall((:slam_pf_get_map, libslamhip), Cint, (Ptr{Cvoid}, Ptr{Int32}, Cint, Ptr{Cdouble}), s.handle, idv, cnt, out))
    out
end

"The local particle with the largest log-weight: (global id, log-weight, pose [x, y, phi], records 5 x max_landmarks)."
function pf_best_particle(s::PFSlamState)
    gid = Ref{Int64}(0)
    logw = Ref{Cdouble}(0.0)
    pose = zeros(Float64, 3)
    lm = zeros(Float64, 5, s.max_landmarks)
    check(ccall((:slam_pf_get_particle, libslamhip), Cint, (Ptr{Cvoid}, Int64, Ref{Int64}, Ref{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                s.handle, -1, gid, logw, pose, lm))
    gid[], logw[], pose, lm
end

# ---- a state handed between the two filters on the device (include/slamhip_handover.h) -------------------------------------------
"""
    to_ekf(pf, ids = nothing; max_landmarks, device = 0) -> (EKFSlamState, info)

The particle filter collapsed into an EKF state (slam_pf_to_ekf): the moment-matched joint Gaussian of the particles over the pose
and the landmarks `ids` (1-based, distinct, any order; `nothing`: every landmark seen so far, ascending), with the pose-landmark and
landmark-landmark cross-covariances that `pf_map` does not have.  Every chosen landmark must be in use in every particle.
`info = (W, Neff, n, N)`.  Whole filter on one rank (`world == 1`); `device` must be the filter's.  The particles are unchanged.
"""
function to_ekf(s::PFSlamState{T}, ids::Union{Nothing,AbstractVector} = nothing;
                max_landmarks::Integer = max(64, 2 * (ids === nothing ? s.max_landmarks : length(ids))), device::Integer = 0) where {T}
    dst = EKFSlamState{T}(zeros(T, 3), zeros(T, 3, 3); max_landmarks = max_landmarks, device = device)
    idv = ids === nothing ? Ptr{Int32}(C_NULL) : (isempty(ids) ? Int32[0] : Vector{Int32}(ids))
    info = zeros(Float64, 4)
    check(ccall((:slam_pf_to_ekf, libslamhip_handover), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}, Cint, Ptr{Cdouble}),
                handle(dst), s.handle, idv, ids === nothing ? 0 : length(ids), info))
    dst, (W = info[1], Neff = info[2], n = Int(info[3]), N = Int(info[4]))
end

"""
    to_particles(state, n, ids = nothing; seed = 0, max_landmarks, device = 0) -> PFSlamState

A particle filter of `n` particles drawn from the EKF state (slam_ekf_to_pf): poses from the vehicle marginal, every landmark `ids`
(`nothing`: all) its conditional given that pose, uniform weights.  Errors with SLAM_E_NOTPD when the vehicle block or a conditional
block is not positive definite (a vehicle known exactly: `set_pose!` and `init_landmarks!`).
"""
function to_particles(st::EKFSlamState{T}, n::Integer, ids::Union{Nothing,AbstractVector} = nothing; seed::Integer = 0,
                      max_landmarks::Integer = max(1, ids === nothing ? div(length(st.x) - 3, 2) : length(ids)),
                      device::Integer = getfield(st, :device)) where {T}
    pf = PFSlamState{T}(n, max_landmarks; seed = seed, device = device)
    idv = ids === nothing ? Ptr{Int32}(C_NULL) : (isempty(ids) ? Int32[0] : Vector{Int32}(ids))
    check(ccall((:slam_ekf_to_pf, libslamhip_handover), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}, Cint),
                pf.handle, handle(st), idv, ids === nothing ? 0 : length(ids)))
    pf
end

# ---- a particle set moved on the device (include/slamhip_pfcopy.h) -------------------------------------------------------------
"(n_local, n_global, first_id, max_landmarks, dtype, RNG step, resample count, seed) and the per-landmark `seen` flags."
function pf_meta(s::PFSlamState)
    out = zeros(Int64, 8)
    seen = zeros(UInt8, s.max_landmarks)
    check(ccall((:slam_pf_get_meta, libslamhip_pfcopy), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{UInt8}), s.handle, out, seen))
    out, seen
end

"The Philox key and the step counter (slam_pf_set_rng): with `pf_meta` and `upload!`, what completes a checkpoint."
function set_rng!(s::PFSlamState, seed::Integer, step::Integer)
    check(ccall((:slam_pf_set_rng, libslamhip_pfcopy), Cint, (Ptr{Cvoid}, UInt64, UInt32), s.handle, seed % UInt64, step))
    s
end

pf_one_rank(s::PFSlamState) = s.world == 1 || error("only a filter that lives wholly on one rank can be copied, selected or resized")

"""
    copy!(dst, src; fill = 0) -> dst

`dst` becomes `src` bit for bit (slam_pf_copy): poses, log-weights as `particles(src)` returns them, every landmark record -- read
where lazy resampling left it, `src` is only read --, the RNG state and the resample count.  Equal particle counts,
`dst.max_landmarks >= src.max_landmarks`; the slots beyond follow `fill` (0: as created, 1: unused, for unknown correspondences).
"""
function Base.copy!(dst::PFSlamState{T}, src::PFSlamState{T}; fill::Integer = 0) where {T}
    pf_one_rank(dst); pf_one_rank(src)
    check(ccall((:slam_pf_copy, libslamhip_pfcopy), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint), dst.handle, src.handle, fill))
    dst
end

"A second filter equal to `s` bit for bit; driven like `s` it stays equal to it.  `max_landmarks` may be larger than `s`'s."
function Base.copy(s::PFSlamState{T}; max_landmarks::Integer = s.max_landmarks, fill::Integer = 0, device::Integer = 0) where {T}
    pf_one_rank(s)
    copy!(PFSlamState{T}(s.n, max_landmarks; device = device), s; fill = fill)
end

"A new filter whose landmark k is slot `ids[k]` of `s` (1-based, distinct, any order) -- slam_pf_select."
function select(s::PFSlamState{T}, ids::AbstractVector{<:Integer}; max_landmarks::Integer = max(1, length(ids)), fill::Integer = 0,
                device::Integer = 0) where {T}
    pf_one_rank(s)
    dst = PFSlamState{T}(s.n, max_landmarks; device = device)
    idv = isempty(ids) ? Int32[0] : Vector{Int32}(ids)
    check(ccall((:slam_pf_select, libslamhip_pfcopy), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}, Cint, Cint),
                dst.handle, s.handle, idv, length(ids), fill))
    dst
end

"""
    resize(s, n, gmax, u0; fill = 0) -> (PFSlamState, ancestors)

A new filter of `n` particles drawn from `s`'s by systematic resampling into `n` slots (slam_pf_resize): uniform weights, the
resample count is `s`'s plus one, `s` is only read.  `gmax`: the largest (normalised) log-weight of `s`; `u0` in [0, 1).
"""
function resize(s::PFSlamState{T}, n::Integer, gmax::Real, u0::Real; fill::Integer = 0, device::Integer = 0) where {T}
    pf_one_rank(s)
    dst = PFSlamState{T}(n, s.max_landmarks; device = device)
    anc = zeros(Int32, n)
    check(ccall((:slam_pf_resize, libslamhip_pfcopy), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cdouble, Cint, Ptr{Int32}),
                dst.handle, s.handle, gmax, u0, fill, anc))
    dst, anc
end

"""
    reserve!(s, max_landmarks; unknown = false) -> s

Make room for `max_landmarks` landmark slots: a new handle is created, the particles are copied into it on the device, it takes
the old handle's place inside `s` and the old one is destroyed.  `unknown`: the new slots are unused records, as a filter with
unknown correspondences needs them.  Objects that borrow the old handle (PathHistory, LandmarkEvidence) must be gone before.
"""
function reserve!(s::PFSlamState{T}, max_landmarks::Integer; unknown::Bool = false, device::Integer = 0) where {T}
    pf_one_rank(s)
    max_landmarks <= s.max_landmarks && return s
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:slam_pf_create, libslamhip), Cint, (Ref{Ptr{Cvoid}}, Cint, Int64, Int64, Int64, Cint, Cint, UInt64),
                h, T === Float32 ? SLAM_F32 : SLAM_F64, s.n, s.n, 0, max_landmarks, device, 0))
    rc = ccall((:slam_pf_copy, libslamhip_pfcopy), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint), h[], s.handle, unknown ? 1 : 0)
    if rc != SLAM_OK
        ccall((:slam_pf_destroy, libslamhip), Cint, (Ptr{Cvoid},), h[])
        check(rc)
    end
    old = s.handle
    s.handle = h[]
    s.max_landmarks = max_landmarks
    ccall((:slam_pf_destroy, libslamhip), Cint, (Ptr{Cvoid},), old)
    s
end

"""
    upload!(s; pose = nothing, logw = nothing, lm = nothing, seen = nothing) -> s

The inverse of `particles` (slam_pf_upload): `pose` n x 3, `logw` n, `lm` n x 5 x max_landmarks in the filter's element type, `seen`
one flag per landmark; `lm` and `seen` go together.  The values are stored as given.
"""
function upload!(s::PFSlamState{T}; pose = nothing, logw = nothing, lm = nothing, seen = nothing) where {T}
    (lm === nothing) == (seen === nothing) || error("lm and seen are given together or not at all")
    p = pose === nothing ? Ptr{Cvoid}(C_NULL) : Matrix{T}(pose)
    w = logw === nothing ? Ptr{Cvoid}(C_NULL) : Vector{T}(logw)
    l = lm === nothing ? Ptr{Cvoid}(C_NULL) : Array{T,3}(lm)
    f = seen === nothing ? Ptr{UInt8}(C_NULL) : Vector{UInt8}(seen .!= 0)
    pose === nothing || size(p) == (s.n, 3) || error("pose must be n x 3")
    logw === nothing || length(w) == s.n || error("logw must have n entries")
    lm === nothing || (size(l) == (s.n, 5, s.max_landmarks) && length(f) == s.max_landmarks) || error("lm must be n x 5 x max_landmarks")
    check(ccall((:slam_pf_upload, libslamhip_pfcopy), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{UInt8}), s.handle, p, w, l, f))
    s
end

"The number of distinct occupied cells of the pose histogram (slam_pf_pose_bins): the k of KLD-sampling."
function pose_bins(s::PFSlamState, cell_xy::Real, cell_phi::Real)
    out = Ref{Int64}(0)
    check(ccall((:slam_pf_pose_bins, libslamhip_pfcopy), Cint, (Ptr{Cvoid}, Cdouble, Cdouble, Ref{Int64}), s.handle, cell_xy, cell_phi, out))
    out[]
end

"The particle count KLD-sampling (Fox 2003) asks for at `k` occupied cells, clamped to [n_min, n_max]; `n_min` for k < 2."
function kld_particle_count(k::Integer; eps::Real = 0.05, z::Real = 2.326, n_min::Integer = 64, n_max::Integer = 1 << 22)
    k < 2 && return Int(n_min)
    a = 2.0 / (9.0 * (k - 1))
    clamp(ceil(Int, (k - 1) / (2.0 * eps) * (1.0 - a + sqrt(a) * z)^3), Int(n_min), Int(n_max))
end

"""
    PathHistory(state, cap)

Per-particle trajectory history of a filter (include/slamhip_path.h): a ring of `cap` records on the device, each a snapshot of
the poses and the ancestors back to the record before.  `record!` makes a record, `resample!(path, gmax, u0)` resamples the
filter with the history following the particles -- a filter with a path object is resampled through it ONLY --, `trace`,
`best_path`, `mean_path` and `survivors` follow the CURRENT particles back through the ring (column 1: the oldest held record).
Only a filter that lives wholly on one rank (`world == 1`).  The object borrows `state` (kept alive through the field).
"""
mutable struct PathHistory
    handle::Ptr{Cvoid}
    state::PFSlamState
    cap::Int
    function PathHistory(s::PFSlamState, cap::Integer)
        s.world == 1 || error("the path history supports only a filter that lives wholly on one rank")
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:slam_pf_path_create, libslamhip_path), Cint, (Ref{Ptr{Cvoid}}, Ptr{Cvoid}, Cint), h, s.handle, cap))
        p = new(h[], s, cap)
        finalizer(p) do ph
            ccall((:slam_pf_path_destroy, libslamhip_path), Cint, (Ptr{Cvoid},), ph.handle)
        end
        return p
    end
end

"One record: the live poses and the composed ancestors of the resamplings since the last record.  Enqueued."
function record!(p::PathHistory)
    check(ccall((:slam_pf_path_record, libslamhip_path), Cint, (Ptr{Cvoid},), p.handle))
    p
end

"slam_pf_resample_local with the history following the particles; `gmax`: the largest (normalised) log-weight, `u0` in [0, 1)."
function resample!(p::PathHistory, gmax::Real, u0::Real)
    check(ccall((:slam_pf_path_resample, libslamhip_path), Cint, (Ptr{Cvoid}, Cdouble, Cdouble), p.handle, gmax, u0))
    p
end

"[records held L, records ever made, cap, resamplings seen]"
function path_info(p::PathHistory)
    out = zeros(Int64, 4)
    check(ccall((:slam_pf_path_info, libslamhip_path), Cint, (Ptr{Cvoid}, Ptr{Int64}), p.handle, out))
    out
end

"The record `k` back (0: the newest): (pose n x 3, ancestors n -- 0-based, the identity where none were stored --, stored?)."
function path_record(p::PathHistory, k::Integer = 0)
    pose = zeros(Float64, p.state.n, 3)                # the library's [3][n], particle index fastest
    anc = zeros(Int32, p.state.n)
    has = Ref{Cint}(0)
    check(ccall((:slam_pf_path_get, libslamhip_path), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Int32}, Ref{Cint}),
                p.handle, k, pose, anc, has))
    pose, anc, has[] != 0
end

"The paths of the current particles `ids` (0-based, at most 4096): 3 x L x length(ids), (x, y, phi), oldest held record first."
function trace(p::PathHistory, ids::AbstractVector)
    idv = Vector{Int64}(ids)
    out = zeros(Float64, 3, max(1, path_info(p)[1]), max(1, length(idv)))
    check(ccall((:slam_pf_path_trace, libslamhip_path), Cint, (Ptr{Cvoid}, Ptr{Int64}, Cint, Ptr{Cdouble}),
                p.handle, idv, length(idv), out))
    out
end

"(index, 3 x L path) of the particle with the largest log-weight (0-based index, the lowest on a tie)."
function best_path(p::PathHistory)
    idx = Ref{Int64}(0)
    out = zeros(Float64, 3, max(1, path_info(p)[1]))
    check(ccall((:slam_pf_path_best, libslamhip_path), Cint, (Ptr{Cvoid}, Ref{Int64}, Ptr{Cdouble}), p.handle, idx, out))
    idx[], out
end

"The mean path under the current weights: 4 x L, (x, y, phi, mean resultant length of the headings) per record."
function mean_path(p::PathHistory)
    out = zeros(Float64, 4, max(1, path_info(p)[1]))
    check(ccall((:slam_pf_path_mean, libslamhip_path), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), p.handle, out))
    out
end

"Distinct particles at each held record that have a descendant among the current particles (the depletion diagnostic)."
function survivors(p::PathHistory)
    out = zeros(Int64, max(1, path_info(p)[1]))
    check(ccall((:slam_pf_path_survivors, libslamhip_path), Cint, (Ptr{Cvoid}, Ptr{Int64}), p.handle, out))
    out
end

"Download: (pose 3 x n ... as n x 3, logw n, lm n x 5 x max_landmarks): the device's SoA arrays, particle index fastest."
function particles(s::PFSlamState{T}) where {T}
    pose = Matrix{T}(undef, s.n, 3)
    logw = Vector{T}(undef, s.n)
    lm = Array{T,3}(undef, s.n, 5, s.max_landmarks)
    check(ccall((:slam_pf_download, libslamhip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), s.handle, pose, logw, lm))
    pose, logw, lm
end

end # module
