# RANSACHIP.jl -- the `ccall` shim a RANSAC.jl maintainer adds to route the hot path of
# RANSAC.jl v0.6.0 through libransac_hip.so (include/ransac_hip.h).
#
# NOT EXECUTED IN THIS REPOSITORY'S CI: the build image has no Julia runtime.  It is written
# against RANSAC.jl v0.6.0's source (src/fitting.jl, src/iterations.jl, src/shapes/*.jl) and the
# C ABI; struct layouts below must stay in sync with include/ransac_hip.h (tests/test_abi.py pins
# sizeof(rh_shape) == 88 and the rh_params field offsets on the C side).
#
# Usage:
#   using RANSAC, RANSACHIP
#   pc  = RANSACCloud(vs, ns, 32)
#   hpc = RANSACHIP.HIPCloud(pc)                      # uploads once; pc stays the source of truth on the host
#   extracted, secs = RANSACHIP.ransac(hpc, params)   # same loop as RANSAC.ransac, GPU hot path
module RANSACHIP

using RANSAC
using RANSAC: FittedShape, FittedPlane, FittedSphere, FittedCylinder, FittedCone,
              ExtractedShape, IterationCandidates, ConfidenceInterval, E,
              recordscore!, findhighestscore, forcefitshapes!, samplepointcloud4!,
              chooseS, prob, updatelevelweight, strt
using StaticArrays

const LIB = get(ENV, "RANSAC_HIP_LIB", joinpath(@__DIR__, "..", "ransac.jl_amd", "libransac_hip.so"))

const RH_PLANE, RH_SPHERE, RH_CYLINDER, RH_CONE = Cint(0), Cint(1), Cint(2), Cint(3)

# typedef struct { int32_t kind; int32_t outwards; double v[10]; } rh_shape;   (88 bytes)
struct RhShape
    kind::Cint
    outwards::Cint
    v::NTuple{10,Cdouble}
end

# rh_params, field for field (include/ransac_hip.h)
struct RhParams
    eps::NTuple{4,Cdouble}
    alpha::NTuple{4,Cdouble}
    cos_alpha::NTuple{4,Cdouble}
    collin_threshold::Cdouble
    parallelthrdeg::Cdouble
    cos_parallelthr::Cdouble
    sphere_par::Cdouble
    minconeopang::Cdouble
    prob_det::Cdouble
    tau::Int64
    itermax::Int64
    drawN::Cint
    minsubsetN::Cint
    extract_s::Cint
    terminate_s::Cint
    n_shape_types::Cint
    shape_types::NTuple{8,Cint}
    score_mode::Cint
    sphere_uses_enabled::Cint
    sampling_streams::Cint
    octree_sampling::Cint
    octree_max_depth::Cint
end

lasterror() = unsafe_string(ccall((:rh_last_error, LIB), Cstring, ()))
check(rc) = rc == 0 ? nothing : error("libransac_hip error $rc: $(lasterror())")

pad10(xs...) = ntuple(i -> i <= length(xs) ? Cdouble(xs[i]) : 0.0, 10)

# FittedShape -> rh_shape.  cos/sin(-opang/2) are computed HERE, with Julia's libm, exactly as
# rodrigues() would (src/utilities.jl:21-22), so the device sees the reference's own constants.
toC(s::FittedPlane) = RhShape(RH_PLANE, 0, pad10(s.point..., s.normal...))
toC(s::FittedSphere) = RhShape(RH_SPHERE, s.outwards, pad10(s.center..., s.radius))
toC(s::FittedCylinder) = RhShape(RH_CYLINDER, s.outwards, pad10(s.axis..., s.center..., s.radius))
toC(s::FittedCone) = RhShape(RH_CONE, s.outwards,
    pad10(s.apex..., s.axis..., s.opang, cos(-s.opang/2), sin(-s.opang/2)))

kindof(::Type{<:FittedPlane}) = RH_PLANE
kindof(::Type{<:FittedSphere}) = RH_SPHERE
kindof(::Type{<:FittedCylinder}) = RH_CYLINDER
kindof(::Type{<:FittedCone}) = RH_CONE

# nested NamedTuple (src/utilities.jl:332-399) -> rh_params; thresholds use Julia's cos / cosd
function toC(p::NamedTuple; score_mode = 0, sphere_uses_enabled = 0, sampling_streams = 0)
    get2(nt, k, d) = haskey(nt, k) ? getfield(nt, k) : d
    sh(name) = get2(p, name, (ϵ = 0.3, α = deg2rad(5)))
    order = (:plane, :sphere, :cylinder, :cone)                       # RH_* kind order
    eps = ntuple(i -> Cdouble(sh(order[i]).ϵ), 4)
    alp = ntuple(i -> Cdouble(sh(order[i]).α), 4)
    it, co = p.iteration, p.common
    sym = Dict(:lengthC => 1, :allcand => 2, :nofminset => 3)
    st = [kindof(T) for T in it.shape_types]
    RhParams(eps, alp, ntuple(i -> cos(alp[i]), 4),
        co.collin_threshold, co.parallelthrdeg, cosd(co.parallelthrdeg),
        get2(get2(p, :sphere, NamedTuple()), :sphere_par, 0.02),
        get2(get2(p, :cone, NamedTuple()), :minconeopang, deg2rad(2)),
        it.prob_det, it.τ, it.itermax, it.drawN, it.minsubsetN,
        sym[it.extract_s], sym[it.terminate_s], length(st),
        ntuple(i -> i <= length(st) ? st[i] : Cint(0), 8), score_mode, sphere_uses_enabled, sampling_streams, 0, 10)
end

"Device-resident twin of a RANSACCloud; `pc` stays authoritative for fits and sampling."
mutable struct HIPCloud{P}
    pc::P
    handle::Ptr{Cvoid}
    function HIPCloud(pc; device = 0)
        # Vector{SVector{3,Float64}} is n x 3 contiguous doubles: passed as is (zero copy on the host side)
        h = Ref{Ptr{Cvoid}}(C_NULL)
        s1 = pc.subsets[1]
        if eltype(eltype(pc.vertices)) == Float32
            # RANSACCloud(...; force_eltype = Float32): Vector{SVector{3,Float32}} as is; scoring and refit then run in binary32
            GC.@preserve pc check(ccall((:rh_cloud_create_f32, LIB), Cint,
                (Ptr{Cfloat}, Ptr{Cfloat}, Int64, Ptr{Int64}, Int64, Cint, Ptr{Ptr{Cvoid}}),
                pointer(reinterpret(Float32, pc.vertices)), pointer(reinterpret(Float32, pc.normals)),
                pc.size, s1, length(s1), device, h))
        else
            GC.@preserve pc check(ccall((:rh_cloud_create, LIB), Cint,
                (Ptr{Cdouble}, Ptr{Cdouble}, Int64, Ptr{Int64}, Int64, Cint, Ptr{Ptr{Cvoid}}),
                pointer(reinterpret(Float64, pc.vertices)), pointer(reinterpret(Float64, pc.normals)),
                pc.size, s1, length(s1), device, h))
        end
        obj = new{typeof(pc)}(pc, h[])
        push_enabled!(obj)
        finalizer(o -> ccall((:rh_cloud_destroy, LIB), Cint, (Ptr{Cvoid},), o.handle), obj)
    end
end

# pc.isenabled::BitVector -> device (same chunk layout), and back
push_enabled!(h::HIPCloud) = check(ccall((:rh_cloud_set_enabled, LIB), Cint,
    (Ptr{Cvoid}, Ptr{UInt64}, Int64), h.handle, h.pc.isenabled.chunks, length(h.pc.isenabled.chunks)))
pull_enabled!(h::HIPCloud) = check(ccall((:rh_cloud_get_enabled, LIB), Cint,
    (Ptr{Cvoid}, Ptr{UInt64}, Int64), h.handle, h.pc.isenabled.chunks, length(h.pc.isenabled.chunks)))

"""
Replacement for `scorecandidates!` (src/fitting.jl:181-190): ONE batched call instead of a
sequential loop.  Legal because nothing reads a score before the loop ends (iterations.jl:99).
`inpoints` are rebuilt from the returned bit masks (subset order), so `IterationCandidates` and
`removeinvalidshapes!` keep working unchanged.
"""
function scorecandidates!(h::HIPCloud, ic::IterationCandidates, candidates, subsetID, params, octree_levels;
                          cparams = toC(params))
    @assert subsetID == 1 "only subset 1 is resident on the device (iterations.jl:95)"
    pc = h.pc
    b = length(candidates)
    if b > 0
        shapes = RhShape[toC(c) for c in candidates]
        counts = Vector{Int32}(undef, b)
        s1 = pc.subsets[1]
        w = cld(length(s1), 64)
        masks = Matrix{UInt64}(undef, w, b)               # column i = row i of the C array
        check(ccall((:rh_score_batch, LIB), Cint,
            (Ptr{Cvoid}, Ptr{RhShape}, Int32, Ref{RhParams}, Ptr{Int32}, Ptr{UInt64}),
            h.handle, shapes, b, cparams, counts, masks))
        for i in 1:b
            bits = BitVector(undef, length(s1))
            copyto!(bits.chunks, view(masks, :, i))
            ip = s1[bits]
            sc = RANSAC.estimatescore(length(s1), pc.size, length(ip))
            pc.levelscore[octree_levels[i]] += E(sc)
            recordscore!(ic, candidates[i], sc, ip)
        end
    end
    empty!(candidates); empty!(octree_levels)
    return nothing
end

"Replacement for `refit` (src/shapes/*.jl): full-cloud scan on the device, ascending indices."
function refit(s::FittedShape, h::HIPCloud, params; cparams = toC(params))
    idx = Vector{Int}(undef, h.pc.size)
    n = Ref{Int64}(0)
    check(ccall((:rh_refit, LIB), Cint,
        (Ptr{Cvoid}, Ref{RhShape}, Ref{RhParams}, Ptr{Int64}, Int64, Ptr{Int64}),
        h.handle, toC(s), cparams, idx, length(idx), n))
    resize!(idx, n[])
    return ExtractedShape(s, idx)
end

"""
The largest connected patch of `refit(s, h, params)` (Schnabel et al. 2007, section 4.4): connectivity on a voxel grid of
size `beta` over the inliers, 26-neighbourhood (`conn26`) or faces only, size counted in points, ties to the component
with the smallest point index (include/ransac_hip.h has the definition).  Returns `(ExtractedShape, n_refit, n_components)`.
"""
function refit_component(s::FittedShape, h::HIPCloud, params, beta; conn26 = true, cparams = toC(params))
    idx = Vector{Int}(undef, h.pc.size)
    n = Ref{Int64}(0); nrefit = Ref{Int64}(0); ncomp = Ref{Int32}(0)
    check(ccall((:rh_refit_component, LIB), Cint,
        (Ptr{Cvoid}, Ref{RhShape}, Ref{RhParams}, Cdouble, Int32, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int32}),
        h.handle, toC(s), cparams, beta, conn26 ? 1 : 0, idx, length(idx), n, nrefit, ncomp))
    resize!(idx, n[])
    return ExtractedShape(s, idx), nrefit[], ncomp[]
end

"With `beta > 0` every extraction of `rh_ransac` on this cloud takes only the largest connected patch of its refit set; `beta <= 0`: off."
set_component_filter!(h::HIPCloud, beta; conn26 = true) = check(ccall((:rh_cloud_set_component_filter, LIB), Cint,
    (Ptr{Cvoid}, Cdouble, Int32), h.handle, beta, conn26 ? 1 : 0))
function component_filter(h::HIPCloud)
    beta = Ref{Cdouble}(0); conn = Ref{Int32}(0)
    check(ccall((:rh_cloud_get_component_filter, LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Int32}), h.handle, beta, conn))
    return beta[], conn[] != 0
end

# rh_extent, field for field (include/ransac_hip.h; 224 bytes)
struct RhExtent
    n::Int64
    kind::Cint
    flags::Cint                       # 1: empty list, 2: no principal direction (fallback frame)
    origin::NTuple{3,Cdouble}
    frame::NTuple{9,Cdouble}          # rows u, v, w
    lo::NTuple{3,Cdouble}
    hi::NTuple{3,Cdouble}
    centroid::NTuple{3,Cdouble}
    lambda::NTuple{3,Cdouble}
    dist_rms::Cdouble
    dist_maxabs::Cdouble
end

"""
Oriented extents and fit residuals of extracted shapes, all in one call on the device (`rh_shape_extents`,
include/ransac_hip.h has the definition): for every `ExtractedShape` the frame its points suggest (rows u, v, w), their
box `lo`..`hi` along it measured from the shape's origin, centroid, scatter, and the rms / largest distance to the shape.
"""
function shape_extents(h::HIPCloud, extracted::AbstractVector{<:ExtractedShape})
    b = length(extracted)
    out = Vector{RhExtent}(undef, b)
    b == 0 && return out
    shapes = RhShape[toC(e.shape) for e in extracted]
    offsets = Int64[0; cumsum(Int64[length(e.inpoints) for e in extracted])]
    idx = isempty(extracted) ? Int64[] : reduce(vcat, (Vector{Int64}(e.inpoints) for e in extracted))
    check(ccall((:rh_shape_extents, LIB), Cint,
        (Ptr{Cvoid}, Ptr{RhShape}, Int32, Ptr{Int64}, Ptr{Int64}, Ptr{RhExtent}),
        h.handle, shapes, b, offsets, idx, out))
    return out
end

"Replacement for `invalidate_indexes!` (src/fitting.jl:197-202): host bits and device bits."
function invalidate_indexes!(h::HIPCloud, indexlist)
    RANSAC.invalidate_indexes!(h.pc, indexlist)
    check(ccall((:rh_invalidate, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Int64), h.handle, indexlist, length(indexlist)))
end

"""
`ransac(pc, params)` (src/iterations.jl:35-162) with the three hot calls swapped; sampling, `fit`,
`findhighestscore`, `prob`, `removeinvalidshapes!` are the reference's own functions.
"""
function ransac(h::HIPCloud, params; reset_rand = false, batched_sampling = false, seed::Integer = 1234)
    pc = h.pc
    reset_rand && RANSAC.Random.seed!(1234)
    it = params.iteration
    cparams = toC(params)
    push_enabled!(h)
    start_time = time_ns()
    candidates = FittedShape[]; scoredshapes = IterationCandidates(); extracted = ExtractedShape[]
    levels = Int[]; sd = Vector{Int}(undef, it.drawN); countcandidates = [0, 0, 0]
    rng = RhRng((UInt64(0), UInt64(0), UInt64(0), UInt64(0)), C_NULL, 0, 0, 0)
    batched_sampling && ccall((:rh_rng_seed, LIB), Cvoid, (Ref{RhRng}, UInt64), rng, UInt64(seed))
    for k in 1:it.itermax
        count(pc.isenabled) < it.τ && break
        if batched_sampling
            # the iteration's minsubsetN calls of samplepointcloud4! as ONE launch (rh_sample_sets) on the library's generator:
            # the same sets and the same number of draws as minsubsetN sequential calls, without a round trip per point
            sets, ok, lev = sample_sets!(h, rng, it.drawN, it.minsubsetN)
            for i in 1:it.minsubsetN
                ok[i] != 0 || continue
                sdi = view(sets, :, i)
                forcefitshapes!(view(pc.vertices, sdi), view(pc.normals, sdi), params, candidates, levels, Int(lev[i]), pc)
            end
        end
        for i in 1:(batched_sampling ? 0 : it.minsubsetN)
            res = samplepointcloud4!(sd, pc, params)
            res[1] || continue
            forcefitshapes!(view(pc.vertices, sd), view(pc.normals, sd), params, candidates, levels, res[2], pc)
        end
        countcandidates[2] += length(candidates)
        scorecandidates!(h, scoredshapes, candidates, 1, params, levels; cparams = cparams)
        countcandidates[3] = k * it.minsubsetN
        countcandidates[1] = length(scoredshapes)
        if length(scoredshapes) > 0
            best = findhighestscore(scoredshapes)
            bestshape = scoredshapes.shapes[best.index]
            scr = E(scoredshapes.scores[best.index])
            if prob(scr, chooseS(countcandidates, it.extract_s), pc.size, it.drawN) > it.prob_det
                ex = refit(bestshape, h, params; cparams = cparams)
                invalidate_indexes!(h, ex.inpoints)
                push!(extracted, ex)
                deleteat!(scoredshapes, best.index)
                RANSAC.removeinvalidshapes!(pc, scoredshapes)
            end
        end
        updatelevelweight(pc)
        prob(it.τ, chooseS(countcandidates, it.terminate_s), pc.size, it.drawN) > it.prob_det && break
    end
    return extracted, trunc((time_ns() - start_time) / 1_000_000_000, digits = 2)
end

"""
`samplepointcloud4!` (src/fitting.jl:383-430) for the `k` minimal sets of an iteration as ONE launch: `rh_sample_sets`.
Returns (`drawN x k` point indices, accept flags, octree levels); `rng` (an `RhRng`, `rh_rng_seed`) is advanced exactly as
`k` sequential calls would advance it.
"""
function sample_sets!(h::HIPCloud, rng, drawN::Integer, k::Integer)
    idx = Matrix{Int64}(undef, drawN, k); ok = Vector{Int32}(undef, k); lev = Vector{Int32}(undef, k)
    check(ccall((:rh_sample_sets, LIB), Cint, (Ptr{Cvoid}, Int32, Ref{RhRng}, Int32, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}),
                h.handle, drawN, rng, k, idx, ok, lev))
    return idx, ok, lev
end

"""
`rh_set_option`: a tuning option for one cloud (or process-wide with `h = nothing`); the library reads no environment
variable.  Keys: "score_path" (0 auto / 1 brute / 2 groups; process-wide, before the cloud is created), "refit_path"
(0 auto / 1 scan / 2 culled), "s4_rows", "unp_words"; `typemin(Int64)` clears a setting.
"""
set_option(h::Union{HIPCloud,Nothing}, key::AbstractString, value::Integer) =
    check(ccall((:rh_set_option, LIB), Cint, (Ptr{Cvoid}, Cstring, Int64), h === nothing ? C_NULL : h.handle, key, value))

# ---- the whole loop on the device: rh_ransac (driver.hip) -------------------------------------
# Mirrors of rh_rng / rh_extracted / rh_result (include/ransac_hip.h).  The index lists live in one
# pinned block owned by the result; they are copied into Julia vectors here and the block goes back
# to the library's pool with rh_result_free.
mutable struct RhRng
    s::NTuple{4,UInt64}
    stream::Ptr{UInt64}
    stream_len::Int64
    stream_pos::Int64
    draws::Int64
end

struct RhExtracted
    shape::RhShape
    n_inpoints::Int64
    inpoints::Ptr{Int64}
    score_E::Cdouble
    iteration::Int64
end

mutable struct RhResult
    shapes::Ptr{RhExtracted}
    n_shapes::Int64
    iterations::Int64
    candidates_scored::Int64
    scored_left::Int64
    seconds::Cdouble
    seconds_score::Cdouble
    seconds_extract::Cdouble
    seconds_host::Cdouble
    seconds_to_last_extraction::Cdouble
    arena::Ptr{Cvoid}
end

fromC(s::RhShape) =
    s.kind == RH_PLANE    ? FittedPlane(SVector(s.v[1:3]...), SVector(s.v[4:6]...)) :
    s.kind == RH_SPHERE   ? FittedSphere(SVector(s.v[1:3]...), s.v[4], s.outwards != 0) :
    s.kind == RH_CYLINDER ? FittedCylinder(SVector(s.v[1:3]...), SVector(s.v[4:6]...), s.v[7], s.outwards != 0) :
                            FittedCone(SVector(s.v[1:3]...), SVector(s.v[4:6]...), s.v[7], s.outwards != 0)

"""
`ransac_device(h, params; seed, sampling_streams)`: the whole `ransac` loop inside the library
(sampling, fits, scoring, refit, invalidation, candidate liveness on the GPU; `sampling_streams = 1`
draws every minimal set from its own counter-based stream so that whole windows of iterations run
on the device).  Same return value as `ransac`.
`mp`: a handle from `mp_open` -- the loop is then run by all processes of that group together on this one
scene (`rh_ransac_mp`: one process per GPU of a node, every one with the same cloud; the minimal sets of every
iteration are dealt round-robin to the ranks); every rank gets the single-process result.
"""
function ransac_device(h::HIPCloud, params; seed::Integer = 1234, sampling_streams::Integer = 1, mp::Ptr{Cvoid} = C_NULL)
    pc = h.pc
    push_enabled!(h)
    cp = Ref(toC(params; sampling_streams = sampling_streams))
    rng = Ref(RhRng((0, 0, 0, 0), C_NULL, 0, 0, 0))
    ccall((:rh_rng_seed, LIB), Cvoid, (Ptr{RhRng}, UInt64), rng, UInt64(seed))
    res = Ref(RhResult(C_NULL, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, C_NULL))
    if eltype(eltype(pc.vertices)) === Float32
        # a Float32 cloud (RANSACCloud(...; force_eltype = Float32), octree.jl:102-109): fits, scoring, liveness and refit in
        # binary32, shapes come back holding Float32 values (all four kinds)
        mp == C_NULL || error("ransac_device: mp is not available on a Float32 cloud")
        GC.@preserve pc check(ccall((:rh_ransac_f32, LIB), Cint,
            (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{RhParams}, Ptr{RhRng}, Ptr{RhResult}),
            h.handle, pointer(reinterpret(Cfloat, pc.vertices)), pointer(reinterpret(Cfloat, pc.normals)), cp, rng, res))
    elseif mp == C_NULL
        GC.@preserve pc check(ccall((:rh_ransac, LIB), Cint,
            (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{RhParams}, Ptr{RhRng}, Ptr{RhResult}),
            h.handle, pointer(reinterpret(Cdouble, pc.vertices)), pointer(reinterpret(Cdouble, pc.normals)), cp, rng, res))
    else
        GC.@preserve pc check(ccall((:rh_ransac_mp, LIB), Cint,
            (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{RhParams}, Ptr{RhRng}, Ptr{Cvoid}, Ptr{RhResult}),
            h.handle, pointer(reinterpret(Cdouble, pc.vertices)), pointer(reinterpret(Cdouble, pc.normals)), cp, rng, mp, res))
    end
    extracted = ExtractedShape[]
    for i in 1:res[].n_shapes
        e = unsafe_load(res[].shapes, i)
        push!(extracted, ExtractedShape(fromC(e.shape), copy(unsafe_wrap(Array, e.inpoints, e.n_inpoints))))
    end
    secs = res[].seconds
    ccall((:rh_result_free, LIB), Cvoid, (Ptr{RhResult},), res)
    pull_enabled!(h)          # the cloud's isenabled now reflects the extractions
    return extracted, secs
end

# the processes of one node that share a scene (collective: every rank calls it with the same name; rank 0 creates
# the shared-memory segment).  `MPI.Comm_rank` / `Comm_size` or the launcher's environment give rank and world.
function mp_open(name::AbstractString, rank::Integer, world::Integer; slot_bytes::Integer = 0)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:rh_mp_open, LIB), Cint, (Cstring, Int32, Int32, Int64, Ptr{Ptr{Cvoid}}), name, rank, world, slot_bytes, h))
    return h[]
end
mp_close(mp::Ptr{Cvoid}) = ccall((:rh_mp_close, LIB), Cint, (Ptr{Cvoid},), mp)

# ---- scoring one batch on all GPUs of a node: candidates are independent (src/fitting.jl:181-190), every rank (one
# Julia process per GPU, each with the same cloud) scores the slice lo:hi of the batch and the library's own RCCL
# all-reduce (sum of the zero-padded Int32 counts over xGMI) gives every rank every count.
#   rank 0:      id = comm_unique_id()      ... send the 128 bytes to the other ranks (MPI.Bcast!, a file, a socket) ...
#   every rank:  comm = comm_create(h, rank, world, id)
#   per batch:   counts = scorecounts_sharded(h, comm, candidates, lo, hi, params)      # length(candidates) counts
function comm_unique_id()
    id = zeros(UInt8, 128)
    check(ccall((:rh_comm_unique_id, LIB), Cint, (Ptr{UInt8},), id))
    return id
end
function comm_create(h::HIPCloud, rank::Integer, world::Integer, id::Vector{UInt8})
    c = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:rh_comm_create, LIB), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{UInt8}, Ptr{Ptr{Cvoid}}), h.handle, rank, world, id, c))
    return c[]
end
comm_destroy(comm::Ptr{Cvoid}) = ccall((:rh_comm_destroy, LIB), Cint, (Ptr{Cvoid},), comm)

function scorecounts_sharded(h::HIPCloud, comm::Ptr{Cvoid}, candidates::Vector{<:FittedShape}, lo::Integer, hi::Integer, params)
    btotal = length(candidates)
    mine = RhShape[toC(c) for c in candidates[lo:hi]]
    cp = Ref(toC(params))
    dsh = Ref{Ptr{Cvoid}}(C_NULL); dcn = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:rh_dev_alloc, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Ptr{Cvoid}}), h.handle, max(1, length(mine)) * sizeof(RhShape), dsh))
    check(ccall((:rh_dev_alloc, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Ptr{Cvoid}}), h.handle, 4 * max(1, btotal), dcn))
    counts = zeros(Int32, btotal)
    try
        check(ccall((:rh_dev_upload, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{RhShape}, Int64), h.handle, dsh[], mine, length(mine) * sizeof(RhShape)))
        check(ccall((:rh_score_batch_allreduce_dev, LIB), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Int32, Ptr{RhParams}, Ptr{Cvoid}),
            h.handle, comm, dsh[], length(mine), lo - 1, btotal, cp, dcn[]))
        check(ccall((:rh_comm_sync, LIB), Cint, (Ptr{Cvoid},), comm))
        check(ccall((:rh_dev_download, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Cvoid}, Int64), h.handle, counts, dcn[], 4 * btotal))
    finally
        ccall((:rh_dev_free, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), h.handle, dsh[])
        ccall((:rh_dev_free, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), h.handle, dcn[])
    end
    return counts
end

# ---- point normals for a cloud without them (rh_estimate_normals; docs/src/ransac.md:13 "PCA for example") ----
# typedef struct { int32_t k; int32_t orient; double radius; double viewpoint[3]; } rh_normals_params;   (40 bytes)
struct RhNormalsParams
    k::Cint
    orient::Cint
    radius::Cdouble
    viewpoint::NTuple{3,Cdouble}
end

"""
    estimatenormals(vertices; k = 16, radius = 0.0, viewpoint = nothing, hints = nothing) -> normals

PCA normals of the k nearest neighbours (the point itself first, ties to the smaller index), computed on the GPU.
`viewpoint` turns every normal towards it, `hints` (one vector per point) along them, neither: the largest component
positive.  Degenerate points get a zero normal.  Float32 vertices give Float32 normals; the result goes into
`RANSACCloud(vertices, normals, subsets)` as is.
"""
function estimatenormals(vertices::AbstractVector{SVector{3,T}}; k::Integer = 16, radius::Real = 0.0,
                         viewpoint = nothing, hints = nothing, device::Integer = 0) where {T<:Union{Float32,Float64}}
    viewpoint !== nothing && hints !== nothing && error("estimatenormals: a viewpoint or hints, not both")
    orient = viewpoint !== nothing ? 1 : (hints !== nothing ? 2 : 0)
    vp = viewpoint === nothing ? (0.0, 0.0, 0.0) : ntuple(i -> Cdouble(viewpoint[i]), 3)
    p = RhNormalsParams(k, orient, radius, vp)
    vs = convert(Vector{SVector{3,T}}, vertices)
    hs = hints === nothing ? nothing : convert(Vector{SVector{3,T}}, hints)
    out = Vector{SVector{3,T}}(undef, length(vs))
    hp = hs === nothing ? Ptr{T}(C_NULL) : pointer(reinterpret(T, hs))
    GC.@preserve vs hs out begin
        if T == Float32
            check(ccall((:rh_estimate_normals_f32, LIB), Cint,
                (Ptr{Cfloat}, Int64, Ref{RhNormalsParams}, Ptr{Cfloat}, Cint, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Int32}),
                pointer(reinterpret(Float32, vs)), length(vs), p, hp, device, pointer(reinterpret(Float32, out)), C_NULL, C_NULL))
        else
            check(ccall((:rh_estimate_normals, LIB), Cint,
                (Ptr{Cdouble}, Int64, Ref{RhNormalsParams}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}),
                pointer(reinterpret(Float64, vs)), length(vs), p, hp, device, pointer(reinterpret(Float64, out)), C_NULL, C_NULL))
        end
    end
    return out
end

# ---- consistent orientation of normals without a viewpoint (rh_orient_normals) ----
# typedef struct { int32_t k; int32_t anchor; double radius; double up[3]; } rh_orient_params;   (40 bytes)
struct RhOrientParams
    k::Cint
    anchor::Cint
    radius::Cdouble
    up::NTuple{3,Cdouble}
end
# typedef struct { int64_t n_vertices, n_edges, n_components, n_tree_edges, n_flipped, n_inconsistent, largest_component;
#                  double min_tree_absdot; } rh_orient_stats;   (64 bytes)
struct RhOrientStats
    n_vertices::Int64
    n_edges::Int64
    n_components::Int64
    n_tree_edges::Int64
    n_flipped::Int64
    n_inconsistent::Int64
    largest_component::Int64
    min_tree_absdot::Cdouble
end

"""
    orientnormals(vertices, normals; k = 16, radius = 0.0, anchor = :top, up = (0, 0, 1)) -> (normals, flip, component, stats)

Turns the normals of a cloud without a viewpoint so that neighbouring normals agree (`rh_orient_normals`,
include/ransac_hip.h has the definition in full): the sign is carried along the minimum spanning forest of the
k-nearest-neighbour graph, edges ordered by descending `|ni . nj|`, then by index.  Every connected part is turned as a
whole: `anchor = :top` makes the normal of its topmost point along `up` point up, `:first` keeps the normal of its
smallest index.  Points with a zero normal take no part.  `flip[i]`: 1 flipped, 0 kept, -1 zero normal; `component[i]`:
1 to M by smallest index, 0 for a zero normal; `stats`: an `RhOrientStats`.
"""
function orientnormals(vertices::AbstractVector{SVector{3,T}}, normals::AbstractVector{SVector{3,T}}; k::Integer = 16,
                       radius::Real = 0.0, anchor::Symbol = :top, up = (0, 0, 1),
                       device::Integer = 0) where {T<:Union{Float32,Float64}}
    anchor in (:first, :top) || error("orientnormals: anchor is :first or :top")
    length(normals) == length(vertices) || error("orientnormals: $(length(normals)) normals for $(length(vertices)) points")
    p = RhOrientParams(k, anchor === :first ? 0 : 1, radius, ntuple(i -> Cdouble(up[i]), 3))
    vs = convert(Vector{SVector{3,T}}, vertices)
    ns = convert(Vector{SVector{3,T}}, normals)
    n = length(vs)
    out = Vector{SVector{3,T}}(undef, n)
    flip = zeros(Int32, max(n, 1))
    comp = zeros(Int32, max(n, 1))
    st = Ref(RhOrientStats(0, 0, 0, 0, 0, 0, 0, Inf))
    GC.@preserve vs ns out flip comp begin
        if T == Float32
            check(ccall((:rh_orient_normals_f32, LIB), Cint,
                (Ptr{Cfloat}, Ptr{Cfloat}, Int64, Ref{RhOrientParams}, Cint, Ptr{Cfloat}, Ptr{Int32}, Ptr{Int32}, Ref{RhOrientStats}),
                pointer(reinterpret(Float32, vs)), pointer(reinterpret(Float32, ns)), n, p, device,
                pointer(reinterpret(Float32, out)), flip, comp, st))
        else
            check(ccall((:rh_orient_normals, LIB), Cint,
                (Ptr{Cdouble}, Ptr{Cdouble}, Int64, Ref{RhOrientParams}, Cint, Ptr{Cdouble}, Ptr{Int32}, Ptr{Int32}, Ref{RhOrientStats}),
                pointer(reinterpret(Float64, vs)), pointer(reinterpret(Float64, ns)), n, p, device,
                pointer(reinterpret(Float64, out)), flip, comp, st))
        end
    end
    return out, resize!(flip, n), resize!(comp, n), st[]
end

# ---- voxel-grid downsampling of a raw cloud (rh_voxel_downsample; the reference leaves thinning to the user) ----
# typedef struct { double beta; int32_t mode; int32_t flags; } rh_voxel_params;   (16 bytes)
struct RhVoxelParams
    beta::Cdouble
    mode::Cint
    flags::Cint
end

"""
    voxeldownsample(vertices, beta; normals = nothing, mode = :centroid, align_normals = false)
        -> (vertices, normals or nothing, first, count, row_of_point)

One point per occupied cell of a grid of width `beta`, rows in the order in which the cells first appear.
`mode = :centroid`: the mean of the cell's points (integer sums: the same bits whatever the order) and the normalised
sum of their normals, each first turned to the side of the cell's first normal with `align_normals`; `mode = :first`:
the cell's first point and normal as they are.  `first` holds the 1-based index of every cell's first point, `count` the
points per cell, `row_of_point[i]` the row of point `i` (0: dropped, a coordinate or normal was not finite).
"""
function voxeldownsample(vertices::AbstractVector{SVector{3,T}}, beta::Real; normals = nothing, mode::Symbol = :centroid,
                         align_normals::Bool = false, device::Integer = 0) where {T<:Union{Float32,Float64}}
    mode in (:first, :centroid) || error("voxeldownsample: mode is :first or :centroid")
    p = RhVoxelParams(beta, mode === :centroid ? 1 : 0, align_normals ? 1 : 0)
    vs = convert(Vector{SVector{3,T}}, vertices)
    ns = normals === nothing ? nothing : convert(Vector{SVector{3,T}}, normals)
    n = length(vs)
    ns === nothing || length(ns) == n || error("voxeldownsample: $(length(ns)) normals for $n points")
    vout = Vector{SVector{3,T}}(undef, n)
    nout = ns === nothing ? nothing : Vector{SVector{3,T}}(undef, n)
    first = Vector{Int64}(undef, n)
    count = Vector{Int32}(undef, n)
    rowof = zeros(Int32, n)
    m = Ref{Int64}(0)
    np = ns === nothing ? Ptr{T}(C_NULL) : pointer(reinterpret(T, ns))
    nop = nout === nothing ? Ptr{T}(C_NULL) : pointer(reinterpret(T, nout))
    GC.@preserve vs ns vout nout first count rowof begin
        if T == Float32
            check(ccall((:rh_voxel_downsample_f32, LIB), Cint,
                (Ptr{Cfloat}, Ptr{Cfloat}, Int64, Ref{RhVoxelParams}, Cint, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Int64}, Ptr{Int32}, Int64,
                 Ptr{Int32}, Ref{Int64}, Ptr{Int64}),
                pointer(reinterpret(Float32, vs)), np, n, p, device, pointer(reinterpret(Float32, vout)), nop, first, count, n,
                rowof, m, C_NULL))
        else
            check(ccall((:rh_voxel_downsample, LIB), Cint,
                (Ptr{Cdouble}, Ptr{Cdouble}, Int64, Ref{RhVoxelParams}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int64}, Ptr{Int32}, Int64,
                 Ptr{Int32}, Ref{Int64}, Ptr{Int64}),
                pointer(reinterpret(Float64, vs)), np, n, p, device, pointer(reinterpret(Float64, vout)), nop, first, count, n,
                rowof, m, C_NULL))
        end
    end
    k = m[]
    return resize!(vout, k), (nout === nothing ? nothing : resize!(nout, k)), resize!(first, k), resize!(count, k), rowof
end

# ---- exact k nearest neighbours and outlier removal of a raw cloud (rh_knn, rh_remove_outliers) ----
# typedef struct { int32_t k; int32_t mode; double std_mul; double radius; double threshold; } rh_outlier_params;   (32 bytes)
struct RhOutlierParams
    k::Cint
    mode::Cint
    std_mul::Cdouble
    radius::Cdouble
    threshold::Cdouble
end
# typedef struct { int64_t n_valid, n_kept; double mu, sigma, tau, nn_median; } rh_outlier_stats;   (48 bytes)
struct RhOutlierStats
    n_valid::Int64
    n_kept::Int64
    mu::Cdouble
    sigma::Cdouble
    tau::Cdouble
    nn_median::Cdouble
end

"""
    knn(vertices, k; radius = 0.0) -> (idx, d2, count)

The `k` (1 to 63) nearest neighbours of every point among the other points, exact: ascending
`d2 = (dx*dx + dy*dy) + dz*dz` in Float64, ties to the smaller index; a duplicate of the point is a neighbour at
distance 0.  `idx` is `k x n` Int32 (column `i` = the neighbours of point `i`, 1-based, 0 past `count[i]`), `d2` the
squared distances (`Inf` there), `count[i]` the neighbours left after `radius > 0` dropped the farther ones.
"""
function knn(vertices::AbstractVector{SVector{3,T}}, k::Integer; radius::Real = 0.0,
             device::Integer = 0) where {T<:Union{Float32,Float64}}
    vs = convert(Vector{SVector{3,T}}, vertices)
    n = length(vs)
    kk = 1 <= k <= 63 ? Int(k) : 1
    idx = zeros(Int32, kk, n)
    d2 = fill(Inf, kk, n)
    count = zeros(Int32, n)
    GC.@preserve vs idx d2 count begin
        if T == Float32
            check(ccall((:rh_knn_f32, LIB), Cint, (Ptr{Cfloat}, Int64, Int32, Cdouble, Cint, Ptr{Int32}, Ptr{Cdouble}, Ptr{Int32}),
                pointer(reinterpret(Float32, vs)), n, k, radius, device, idx, d2, count))
        else
            check(ccall((:rh_knn, LIB), Cint, (Ptr{Cdouble}, Int64, Int32, Cdouble, Cint, Ptr{Int32}, Ptr{Cdouble}, Ptr{Int32}),
                pointer(reinterpret(Float64, vs)), n, k, radius, device, idx, d2, count))
        end
    end
    return idx, d2, count
end

"""
    removeoutliers(vertices; k = 16, std_mul = 2.0, mode = :statistical, radius = 0.0, threshold = nothing, normals = nothing)
        -> (vertices, normals or nothing, kept_idx, stats)

Drops the stray points of a raw cloud (`rh_remove_outliers`, include/ransac_hip.h has the definition in full).  With
`m[i]` the mean distance of point `i` to its `k` nearest neighbours (within `radius` when it is positive):
`:statistical` keeps `m[i] <= mu + std_mul * sigma`, `:absolute` keeps `m[i] <= threshold`, `:radius` keeps the points
with at least `k` other points within `radius`.  `kept_idx`: the kept points' indices, ascending; `stats`: an
`RhOutlierStats` (`nn_median` is the cloud's median nearest-neighbour distance).
"""
function removeoutliers(vertices::AbstractVector{SVector{3,T}}; k::Integer = 16, std_mul::Real = 2.0, mode::Symbol = :statistical,
                        radius::Real = 0.0, threshold = nothing, normals = nothing,
                        device::Integer = 0) where {T<:Union{Float32,Float64}}
    mode in (:statistical, :absolute, :radius) || error("removeoutliers: mode is :statistical, :absolute or :radius")
    mode === :absolute && threshold === nothing && error("removeoutliers: mode :absolute needs a threshold")
    m = mode === :statistical ? 0 : (mode === :absolute ? 1 : 2)
    p = RhOutlierParams(k, m, std_mul, radius, threshold === nothing ? 0.0 : threshold)
    vs = convert(Vector{SVector{3,T}}, vertices)
    n = length(vs)
    normals === nothing || length(normals) == n || error("removeoutliers: $(length(normals)) normals for $n points")
    keep = zeros(UInt8, n)
    idx = zeros(Int32, max(n, 1))
    nk = Ref{Int64}(0)
    st = Ref(RhOutlierStats(0, 0, 0.0, 0.0, 0.0, 0.0))
    GC.@preserve vs keep idx begin
        if T == Float32
            check(ccall((:rh_remove_outliers_f32, LIB), Cint,
                (Ptr{Cfloat}, Int64, Ref{RhOutlierParams}, Cint, Ptr{UInt8}, Ptr{Int32}, Int64, Ref{Int64}, Ptr{Cdouble}, Ref{RhOutlierStats}),
                pointer(reinterpret(Float32, vs)), n, p, device, keep, idx, n, nk, C_NULL, st))
        else
            check(ccall((:rh_remove_outliers, LIB), Cint,
                (Ptr{Cdouble}, Int64, Ref{RhOutlierParams}, Cint, Ptr{UInt8}, Ptr{Int32}, Int64, Ref{Int64}, Ptr{Cdouble}, Ref{RhOutlierStats}),
                pointer(reinterpret(Float64, vs)), n, p, device, keep, idx, n, nk, C_NULL, st))
        end
    end
    resize!(idx, nk[])
    return vs[idx], (normals === nothing ? nothing : normals[idx]), idx, st[]
end

# ---- density-based clustering of a raw cloud (rh_cluster) ----
# typedef struct { double eps; int32_t min_pts, min_size, order, reserved; } rh_cluster_params;   (24 bytes)
struct RhClusterParams
    eps::Cdouble
    min_pts::Cint
    min_size::Cint
    order::Cint
    reserved::Cint
end
# typedef struct { int64_t n_clusters, n_core, n_border, n_noise, n_small, largest; } rh_cluster_stats;   (48 bytes)
struct RhClusterStats
    n_clusters::Int64
    n_core::Int64
    n_border::Int64
    n_noise::Int64
    n_small::Int64
    largest::Int64
end

"""
    cluster(vertices, eps; min_pts = 8, min_size = 1, order = :index) -> (labels, kind, counts, offsets, idx, stats)

Splits a raw cloud into its spatially connected parts (`rh_cluster`: DBSCAN, include/ransac_hip.h has the definition in
full).  Points are neighbours when `d2 <= eps*eps`; a point with at least `min_pts` points within `eps`, itself included,
is a core point; clusters are the connected components of the core points, any other point joins the cluster of its
nearest core neighbour (ties to the smaller index) or is noise, and clusters below `min_size` points become noise.
`min_pts = 1` is Euclidean cluster extraction.  `labels[i]`: 0 for noise, else 1 to M, numbered by the smallest core
point's index (`:index`) or by descending size (`:size`); `kind[i]`: 0 noise, 1 border, 2 core; `counts[1]` the noise
points, `counts[l + 1]` those of cluster `l`; `idx[offsets[l + 1] + 1 : offsets[l + 2]]` the points of label `l`,
ascending; `stats`: an `RhClusterStats`.
"""
function cluster(vertices::AbstractVector{SVector{3,T}}, eps::Real; min_pts::Integer = 8, min_size::Integer = 1,
                 order::Symbol = :index, device::Integer = 0) where {T<:Union{Float32,Float64}}
    order in (:index, :size) || error("cluster: order is :index or :size")
    p = RhClusterParams(eps, min_pts, min_size, order === :index ? 0 : 1, 0)
    vs = convert(Vector{SVector{3,T}}, vertices)
    n = length(vs)
    labels = zeros(Int32, max(n, 1))
    kind = zeros(UInt8, max(n, 1))
    counts = zeros(Int64, n + 1)
    offsets = zeros(Int64, n + 2)
    idx = zeros(Int64, max(n, 1))
    m = Ref{Int64}(0)
    st = Ref(RhClusterStats(0, 0, 0, 0, 0, 0))
    GC.@preserve vs labels kind counts offsets idx begin
        if T == Float32
            check(ccall((:rh_cluster_f32, LIB), Cint,
                (Ptr{Cfloat}, Int64, Ref{RhClusterParams}, Cint, Ptr{Int32}, Ptr{UInt8}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64},
                 Ref{Int64}, Ref{RhClusterStats}),
                pointer(reinterpret(Float32, vs)), n, p, device, labels, kind, n, counts, offsets, idx, m, st))
        else
            check(ccall((:rh_cluster, LIB), Cint,
                (Ptr{Cdouble}, Int64, Ref{RhClusterParams}, Cint, Ptr{Int32}, Ptr{UInt8}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64},
                 Ref{Int64}, Ref{RhClusterStats}),
                pointer(reinterpret(Float64, vs)), n, p, device, labels, kind, n, counts, offsets, idx, m, st))
        end
    end
    return resize!(labels, n), resize!(kind, n), resize!(counts, m[] + 1), resize!(offsets, m[] + 2), resize!(idx, n), st[]
end

# ---- region growing by smoothness for a cloud with normals (rh_segment_smooth) ----
# typedef struct { int32_t k, flags; double radius, cos_angle, curv_max, dist_max; int32_t min_size, order; } rh_segment_params;   (48 bytes)
struct RhSegmentParams
    k::Cint
    flags::Cint
    radius::Cdouble
    cos_angle::Cdouble
    curv_max::Cdouble
    dist_max::Cdouble
    min_size::Cint
    order::Cint
end
# typedef struct { int64_t n_regions, n_seed, n_border, n_unassigned, n_invalid, n_small, largest; } rh_segment_stats;   (56 bytes)
struct RhSegmentStats
    n_regions::Int64
    n_seed::Int64
    n_border::Int64
    n_unassigned::Int64
    n_invalid::Int64
    n_small::Int64
    largest::Int64
end

"""
    segment_smooth(vertices, normals; curvature = nothing, k = 16, radius = 0, angle = deg2rad(25), curv_max = 0.05,
                   dist_max = 0, unsigned = false, min_size = 1, order = :size)
        -> (labels, kind, counts, offsets, idx, stats)

Splits a cloud with normals into its smooth sheets (`rh_segment_smooth`: region growing by smoothness, stated so that
nothing depends on an order; include/ransac_hip.h has the definition in full).  Two points are linked when one is among
the other's `k` nearest neighbours, their normals differ by at most `angle` (radians; `unsigned`: up to sign) and, with
`dist_max > 0`, each lies within `dist_max` of the other's tangent plane.  A point whose curvature is at most `curv_max`
is a seed (every point with a normal, without `curvature`); regions are the connected components of the seeds, any other
point joins the region of its nearest linked seed (ties to the smaller index) or has no label, and neither have regions
below `min_size` points nor points whose normal is (0, 0, 0).  The cosine of `angle` is taken here.  `labels[i]`: 0 for
none, else 1 to M, by descending size (`:size`) or by the smallest seed's index (`:index`); `kind[i]`: 0 none, 1 border,
2 seed; `counts`, `offsets` and `idx` as in `cluster`; `stats`: an `RhSegmentStats`.
"""
function segment_smooth(vertices::AbstractVector{SVector{3,T}}, normals::AbstractVector{SVector{3,T}};
                        curvature::Union{Nothing,AbstractVector{T}} = nothing, k::Integer = 16, radius::Real = 0.0,
                        angle::Real = deg2rad(25.0), curv_max::Real = 0.05, dist_max::Real = 0.0, unsigned::Bool = false,
                        min_size::Integer = 1, order::Symbol = :size, device::Integer = 0) where {T<:Union{Float32,Float64}}
    order in (:index, :size) || error("segment_smooth: order is :index or :size")
    length(normals) == length(vertices) || error("segment_smooth: as many normals as vertices")
    curvature === nothing || length(curvature) == length(vertices) || error("segment_smooth: as many curvatures as vertices")
    p = RhSegmentParams(k, unsigned ? 1 : 0, radius, cos(Float64(angle)), curv_max, dist_max, min_size, order === :index ? 0 : 1)
    vs = convert(Vector{SVector{3,T}}, vertices)
    ns = convert(Vector{SVector{3,T}}, normals)
    cs = curvature === nothing ? T[] : convert(Vector{T}, curvature)
    n = length(vs)
    labels = zeros(Int32, max(n, 1))
    kind = zeros(UInt8, max(n, 1))
    counts = zeros(Int64, n + 1)
    offsets = zeros(Int64, n + 2)
    idx = zeros(Int64, max(n, 1))
    m = Ref{Int64}(0)
    st = Ref(RhSegmentStats(0, 0, 0, 0, 0, 0, 0))
    GC.@preserve vs ns cs labels kind counts offsets idx begin
        pc = curvature === nothing ? Ptr{T}(C_NULL) : pointer(cs)
        if T == Float32
            check(ccall((:rh_segment_smooth_f32, LIB), Cint,
                (Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Ref{RhSegmentParams}, Cint, Ptr{Int32}, Ptr{UInt8}, Int64, Ptr{Int64},
                 Ptr{Int64}, Ptr{Int64}, Ref{Int64}, Ref{RhSegmentStats}),
                pointer(reinterpret(Float32, vs)), pointer(reinterpret(Float32, ns)), pc, n, p, device, labels, kind, n, counts,
                offsets, idx, m, st))
        else
            check(ccall((:rh_segment_smooth, LIB), Cint,
                (Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Ref{RhSegmentParams}, Cint, Ptr{Int32}, Ptr{UInt8}, Int64, Ptr{Int64},
                 Ptr{Int64}, Ptr{Int64}, Ref{Int64}, Ref{RhSegmentStats}),
                pointer(reinterpret(Float64, vs)), pointer(reinterpret(Float64, ns)), pc, n, p, device, labels, kind, n, counts,
                offsets, idx, m, st))
        end
    end
    return resize!(labels, n), resize!(kind, n), resize!(counts, m[] + 1), resize!(offsets, m[] + 2), resize!(idx, n), st[]
end

# ---- nearest neighbours of query points in another cloud, and cloud distances (rh_knn_query, rh_cloud_distance) ----
# typedef struct { double radius; double threshold; int32_t metric; int32_t reserved; } rh_distance_params;   (24 bytes)
struct RhDistanceParams
    radius::Cdouble
    threshold::Cdouble
    metric::Cint
    reserved::Cint
end
# typedef struct { int64_t n_valid, n_within, argmax; double mean, rms, max, median; } rh_distance_stats;   (56 bytes)
struct RhDistanceStats
    n_valid::Int64
    n_within::Int64
    argmax::Int64
    mean::Cdouble
    rms::Cdouble
    max::Cdouble
    median::Cdouble
end

"""
    knn_query(reference, queries, k; radius = 0.0) -> (idx, d2, count)

The `k` (1 to 63) nearest points of `reference` for every point of `queries`, exact: ascending
`d2 = (dx*dx + dy*dy) + dz*dz` in Float64, ties to the smaller reference index; no point is left out, so a reference
point equal to the query is its first neighbour at 0 (`knn` is the call for a cloud's own points).  `idx` is `k x m`
Int32 (column `j` = the neighbours of query `j`, 1-based rows of `reference`, 0 past `count[j]`), `d2` the squared
distances (`Inf` there), `count[j]` the neighbours left after `radius > 0` dropped the farther ones.
"""
function knn_query(reference::AbstractVector{SVector{3,T}}, queries::AbstractVector{SVector{3,T}}, k::Integer;
                   radius::Real = 0.0, device::Integer = 0) where {T<:Union{Float32,Float64}}
    rs = convert(Vector{SVector{3,T}}, reference)
    qs = convert(Vector{SVector{3,T}}, queries)
    n, m = length(rs), length(qs)
    kk = 1 <= k <= 63 ? Int(k) : 1
    idx = zeros(Int32, kk, m)
    d2 = fill(Inf, kk, m)
    count = zeros(Int32, m)
    GC.@preserve rs qs idx d2 count begin
        if T == Float32
            check(ccall((:rh_knn_query_f32, LIB), Cint,
                (Ptr{Cfloat}, Int64, Ptr{Cfloat}, Int64, Int32, Cdouble, Cint, Ptr{Int32}, Ptr{Cdouble}, Ptr{Int32}),
                pointer(reinterpret(Float32, rs)), n, pointer(reinterpret(Float32, qs)), m, k, radius, device, idx, d2, count))
        else
            check(ccall((:rh_knn_query, LIB), Cint,
                (Ptr{Cdouble}, Int64, Ptr{Cdouble}, Int64, Int32, Cdouble, Cint, Ptr{Int32}, Ptr{Cdouble}, Ptr{Int32}),
                pointer(reinterpret(Float64, rs)), n, pointer(reinterpret(Float64, qs)), m, k, radius, device, idx, d2, count))
        end
    end
    return idx, d2, count
end

"""
    cloud_distance(reference, queries; normals = nothing, radius = 0.0, threshold = Inf, metric = nothing)
        -> (dist, nn_idx, stats)

How far every point of `queries` lies from the cloud `reference` (`rh_cloud_distance`, include/ransac_hip.h has the
definition in full).  `metric = :point`: the distance to the nearest reference point; `:plane`: `|(q - r) . n|` with `r`
that point and `n` its entry of `normals` (the reference's, used as given); the default is `:plane` when normals are
given.  `radius > 0`: a query without a reference point within it is not valid, `dist[j] = Inf`, `nn_idx[j] = 0`.
`stats`: an `RhDistanceStats` over the valid queries (`max` is the one-sided Hausdorff distance; the symmetric measures
are two calls with the clouds exchanged).
"""
function cloud_distance(reference::AbstractVector{SVector{3,T}}, queries::AbstractVector{SVector{3,T}}; normals = nothing,
                        radius::Real = 0.0, threshold::Real = Inf, metric = nothing,
                        device::Integer = 0) where {T<:Union{Float32,Float64}}
    metric === nothing && (metric = normals === nothing ? :point : :plane)
    metric in (:point, :plane) || error("cloud_distance: metric is :point or :plane")
    rs = convert(Vector{SVector{3,T}}, reference)
    qs = convert(Vector{SVector{3,T}}, queries)
    ns = normals === nothing ? nothing : convert(Vector{SVector{3,T}}, normals)
    n, m = length(rs), length(qs)
    ns === nothing || length(ns) == n || error("cloud_distance: $(length(ns)) normals for $n reference points")
    p = RhDistanceParams(radius, threshold, metric === :point ? 0 : 1, 0)
    dist = fill(Inf, m)
    nn = zeros(Int32, m)
    st = Ref(RhDistanceStats(0, 0, 0, 0.0, 0.0, 0.0, 0.0))
    GC.@preserve rs qs ns dist nn begin
        if T == Float32
            check(ccall((:rh_cloud_distance_f32, LIB), Cint,
                (Ptr{Cfloat}, Ptr{Cfloat}, Int64, Ptr{Cfloat}, Int64, Ref{RhDistanceParams}, Cint, Ptr{Cdouble}, Ptr{Int32}, Ref{RhDistanceStats}),
                pointer(reinterpret(Float32, rs)), ns === nothing ? C_NULL : pointer(reinterpret(Float32, ns)), n,
                pointer(reinterpret(Float32, qs)), m, p, device, dist, nn, st))
        else
            check(ccall((:rh_cloud_distance, LIB), Cint,
                (Ptr{Cdouble}, Ptr{Cdouble}, Int64, Ptr{Cdouble}, Int64, Ref{RhDistanceParams}, Cint, Ptr{Cdouble}, Ptr{Int32}, Ref{RhDistanceStats}),
                pointer(reinterpret(Float64, rs)), ns === nothing ? C_NULL : pointer(reinterpret(Float64, ns)), n,
                pointer(reinterpret(Float64, qs)), m, p, device, dist, nn, st))
        end
    end
    return dist, nn, st[]
end

# ---- rigid registration of one cloud onto another (rh_register) ----
# typedef struct { double radius, rot_tol, trans_tol; int32_t metric, max_iter; } rh_register_params;   (32 bytes)
struct RhRegisterParams
    radius::Cdouble
    rot_tol::Cdouble
    trans_tol::Cdouble
    metric::Cint
    max_iter::Cint
end
# typedef struct { int32_t status, iterations; int64_t n_valid; double rms; } rh_register_result;   (24 bytes)
struct RhRegisterResult
    status::Cint
    iterations::Cint
    n_valid::Int64
    rms::Cdouble
end
const REG_STATUS = (:converged, :max_iter, :degenerate, :too_few)

"""
    register(reference, queries; normals = nothing, metric = nothing, radius = 0.0, max_iter = 50, rot_tol = 1e-9,
             trans_tol = 1e-9, init = nothing) -> (T, info)

The rigid motion that brings `queries` onto `reference` by iterative closest point (`rh_register`, include/ransac_hip.h
has the definition in full).  `metric = :point` minimises the distance to the nearest reference point, `:plane` the
distance to its tangent plane with `normals` the reference's; the default is `:plane` when normals are given.
`radius > 0`: a query without a reference point within it takes no part in an iteration.  `init`: a 3x4 or 4x4 start.
`T` is a 4x4 `Matrix{Float64}` with `x' = T[1:3, 1:3] * x + T[1:3, 4]`; `info` a named tuple `status` (`:converged`,
`:max_iter`, `:degenerate`, `:too_few`), `iterations`, `n_valid`, `rms` and the per-iteration `n_valid_it`, `rms_it`.
"""
function register(reference::AbstractVector{SVector{3,T}}, queries::AbstractVector{SVector{3,T}}; normals = nothing,
                  metric = nothing, radius::Real = 0.0, max_iter::Integer = 50, rot_tol::Real = 1e-9, trans_tol::Real = 1e-9,
                  init = nothing, device::Integer = 0) where {T<:Union{Float32,Float64}}
    metric === nothing && (metric = normals === nothing ? :point : :plane)
    metric in (:point, :plane) || error("register: metric is :point or :plane")
    rs = convert(Vector{SVector{3,T}}, reference)
    qs = convert(Vector{SVector{3,T}}, queries)
    ns = normals === nothing ? nothing : convert(Vector{SVector{3,T}}, normals)
    n, m = length(rs), length(qs)
    ns === nothing || length(ns) == n || error("register: $(length(ns)) normals for $n reference points")
    ini = init === nothing ? nothing : collect(Float64, permutedims(Matrix{Float64}(init)[1:3, 1:4]))   # row-major 3x4
    p = RhRegisterParams(radius, rot_tol, trans_tol, metric === :point ? 0 : 1, max_iter)
    out = zeros(Float64, 4, 3)                   # the library's row-major 3x4, read here column by column
    hist = 1 <= max_iter <= 1000 ? Int(max_iter) : 1
    nv = zeros(Int32, hist)
    rms = zeros(Float64, hist)
    res = Ref(RhRegisterResult(0, 0, 0, 0.0))
    GC.@preserve rs qs ns ini out nv rms begin
        if T == Float32
            check(ccall((:rh_register_f32, LIB), Cint,
                (Ptr{Cfloat}, Ptr{Cfloat}, Int64, Ptr{Cfloat}, Int64, Ref{RhRegisterParams}, Ptr{Cdouble}, Cint, Ptr{Cdouble},
                 Ref{RhRegisterResult}, Ptr{Int32}, Ptr{Cdouble}),
                pointer(reinterpret(Float32, rs)), ns === nothing ? C_NULL : pointer(reinterpret(Float32, ns)), n,
                pointer(reinterpret(Float32, qs)), m, p, ini === nothing ? C_NULL : pointer(ini), device, out, res, nv, rms))
        else
            check(ccall((:rh_register, LIB), Cint,
                (Ptr{Cdouble}, Ptr{Cdouble}, Int64, Ptr{Cdouble}, Int64, Ref{RhRegisterParams}, Ptr{Cdouble}, Cint, Ptr{Cdouble},
                 Ref{RhRegisterResult}, Ptr{Int32}, Ptr{Cdouble}),
                pointer(reinterpret(Float64, rs)), ns === nothing ? C_NULL : pointer(reinterpret(Float64, ns)), n,
                pointer(reinterpret(Float64, qs)), m, p, ini === nothing ? C_NULL : pointer(ini), device, out, res, nv, rms))
        end
    end
    r = res[]
    it = Int(r.iterations)
    Tm = vcat(permutedims(out), [0.0 0.0 0.0 1.0])
    return Tm, (status = REG_STATUS[r.status + 1], iterations = it, n_valid = r.n_valid, rms = r.rms,
                n_valid_it = nv[1:it], rms_it = rms[1:it])
end

# ---- global registration without a start (rh_describe, rh_match_features, rh_register_global) ----
const DESC_DIM = 33
# typedef struct { int32_t trials, reserved; uint64_t seed; double tau, edge_ratio, min_edge; } rh_global_params;   (40 bytes)
struct RhGlobalParams
    trials::Cint
    reserved::Cint
    seed::UInt64
    tau::Cdouble
    edge_ratio::Cdouble
    min_edge::Cdouble
end
# typedef struct { int32_t status, best_trial, best_count, n_valid_trials; } rh_global_result;   (16 bytes)
struct RhGlobalResult
    status::Cint
    best_trial::Cint
    best_count::Cint
    n_valid_trials::Cint
end
const GLOB_STATUS = (:ok, :no_trial)

"""
    describe(vertices, normals; k = 32, radius = 0.0) -> (desc, count)

An integer point-feature histogram per point (`rh_describe`, include/ransac_hip.h has the definition in full): `desc` is a
33 x n `Matrix{UInt16}` (column `i` = the descriptor of point `i`, values 0 .. 7938), `count` the neighbours per point.
The normals are used as given.
"""
function describe(vertices::AbstractVector{SVector{3,T}}, normals::AbstractVector{SVector{3,T}}; k::Integer = 32,
                  radius::Real = 0.0, device::Integer = 0) where {T<:Union{Float32,Float64}}
    vs = convert(Vector{SVector{3,T}}, vertices)
    ns = convert(Vector{SVector{3,T}}, normals)
    n = length(vs)
    length(ns) == n || error("describe: $(length(ns)) normals for $n points")
    desc = zeros(UInt16, DESC_DIM, n)
    count = zeros(Int32, n)
    GC.@preserve vs ns desc count begin
        if T == Float32
            check(ccall((:rh_describe_f32, LIB), Cint, (Ptr{Cfloat}, Ptr{Cfloat}, Int64, Int32, Cdouble, Cint, Ptr{UInt16}, Ptr{Int32}),
                pointer(reinterpret(Float32, vs)), pointer(reinterpret(Float32, ns)), n, k, radius, device, desc, count))
        else
            check(ccall((:rh_describe, LIB), Cint, (Ptr{Cdouble}, Ptr{Cdouble}, Int64, Int32, Cdouble, Cint, Ptr{UInt16}, Ptr{Int32}),
                pointer(reinterpret(Float64, vs)), pointer(reinterpret(Float64, ns)), n, k, radius, device, desc, count))
        end
    end
    return desc, count
end

"""
    match_features(ref_desc, qry_desc; mutual = false) -> (idx, dist)

For every column of `qry_desc` the column of `ref_desc` (both 33 x rows `Matrix{UInt16}`, as `describe` returns them) with
the smallest sum of squared differences, ties to the smaller index (`rh_match_features`): `idx` 1-based `Int32`, `dist` the
sums.  `mutual`: an entry is 0 unless the query is in turn the best query of its reference column.
"""
function match_features(ref_desc::Matrix{UInt16}, qry_desc::Matrix{UInt16}; mutual::Bool = false, device::Integer = 0)
    size(ref_desc, 1) == DESC_DIM && size(qry_desc, 1) == DESC_DIM || error("match_features: descriptors are 33 x rows")
    n, m = size(ref_desc, 2), size(qry_desc, 2)
    idx = zeros(Int32, m)
    dist = zeros(UInt32, m)
    check(ccall((:rh_match_features, LIB), Cint, (Ptr{UInt16}, Int64, Ptr{UInt16}, Int64, Int32, Cint, Ptr{Int32}, Ptr{UInt32}),
        ref_desc, n, qry_desc, m, mutual ? 1 : 0, device, idx, dist))
    return idx, dist
end

"""
    register_global(reference, queries, corr_qry, corr_ref; tau, trials = 20000, seed = 0, edge_ratio = 0.9, min_edge = 0.0,
                    triples = nothing) -> (T, info)

The rigid motion of `queries` onto `reference` that most of the correspondences `(corr_qry[i], corr_ref[i])` (1-based)
agree with, by RANSAC over triples of them (`rh_register_global`, include/ransac_hip.h has the definition in full).
`triples`: a 3 x trials `Matrix{Int32}`, 0-based into the correspondences, instead of the draws from `seed`.  `T` is a 4x4
`Matrix{Float64}`, a start for `register`; `info` a named tuple `status` (`:ok`, `:no_trial`), `best_trial` (0-based),
`best_count`, `n_valid_trials` and `counts`.  `tau`: about 1.5 point spacings.
"""
function register_global(reference::AbstractVector{SVector{3,T}}, queries::AbstractVector{SVector{3,T}},
                         corr_qry::AbstractVector{<:Integer}, corr_ref::AbstractVector{<:Integer}; tau::Real, trials::Integer = 20000,
                         seed::Integer = 0, edge_ratio::Real = 0.9, min_edge::Real = 0.0, triples = nothing,
                         device::Integer = 0) where {T<:Union{Float32,Float64}}
    rs = convert(Vector{SVector{3,T}}, reference)
    qs = convert(Vector{SVector{3,T}}, queries)
    cq = convert(Vector{Int32}, corr_qry)
    cr = convert(Vector{Int32}, corr_ref)
    length(cq) == length(cr) || error("register_global: $(length(cq)) query and $(length(cr)) reference indices")
    tri = triples === nothing ? nothing : convert(Matrix{Int32}, triples)
    tri === nothing || (size(tri, 1) == 3 || error("register_global: triples are 3 x trials"); trials = size(tri, 2))
    p = RhGlobalParams(trials, 0, seed, tau, edge_ratio, min_edge)
    out = zeros(Float64, 4, 3)                   # the library's row-major 3x4, read here column by column
    counts = zeros(Int32, 1 <= trials <= (1 << 20) ? Int(trials) : 1)
    res = Ref(RhGlobalResult(0, 0, 0, 0))
    GC.@preserve rs qs cq cr tri out counts begin
        if T == Float32
            check(ccall((:rh_register_global_f32, LIB), Cint,
                (Ptr{Cfloat}, Int64, Ptr{Cfloat}, Int64, Ptr{Int32}, Ptr{Int32}, Int64, Ref{RhGlobalParams}, Ptr{Int32}, Cint,
                 Ptr{Cdouble}, Ref{RhGlobalResult}, Ptr{Int32}),
                pointer(reinterpret(Float32, rs)), length(rs), pointer(reinterpret(Float32, qs)), length(qs), cq, cr, length(cq), p,
                tri === nothing ? C_NULL : pointer(tri), device, out, res, counts))
        else
            check(ccall((:rh_register_global, LIB), Cint,
                (Ptr{Cdouble}, Int64, Ptr{Cdouble}, Int64, Ptr{Int32}, Ptr{Int32}, Int64, Ref{RhGlobalParams}, Ptr{Int32}, Cint,
                 Ptr{Cdouble}, Ref{RhGlobalResult}, Ptr{Int32}),
                pointer(reinterpret(Float64, rs)), length(rs), pointer(reinterpret(Float64, qs)), length(qs), cq, cr, length(cq), p,
                tri === nothing ? C_NULL : pointer(tri), device, out, res, counts))
        end
    end
    r = res[]
    Tm = vcat(permutedims(out), [0.0 0.0 0.0 1.0])
    return Tm, (status = GLOB_STATUS[r.status + 1], best_trial = Int(r.best_trial), best_count = Int(r.best_count),
                n_valid_trials = Int(r.n_valid_trials), counts = counts)
end

_assign_shape(x::ExtractedShape) = toC(x.shape)
_assign_shape(x::FittedShape) = toC(x)

"""
    assign_points(vertices, normals, shapes, params; use_normals = true, device = 0) -> (labels, dist, counts, offsets, idx)

Every point labelled with its nearest compatible shape (`rh_assign_points`, include/ransac_hip.h has the definition):
`labels[i] = j` for the shape `shapes[j]` (`FittedShape`s or `ExtractedShape`s, at most 1024) that claims point `i` -- the
test of `refit`, distance < eps and angle within alpha -- at the smallest distance, ties to the earlier shape; 0 when none
does.  `normals = nothing` or `use_normals = false`: the distance alone decides.  `dist[i]`: the winner's distance, -1 for
label 0; `counts[1]` the unlabelled points, `counts[j + 1]` those of shape `j`; `idx[offsets[k] + 1 : offsets[k + 1]]` the
points of label `k - 1`, ascending (label 0 first).  Float32 points are promoted exactly; no cloud is needed.
"""
function assign_points(vertices::AbstractVector{SVector{3,T}}, normals, shapes, params; use_normals::Bool = true,
                       device::Integer = 0, cparams = toC(params)) where {T<:Union{Float32,Float64}}
    vs = convert(Vector{SVector{3,T}}, vertices)
    ns = normals === nothing ? nothing : convert(Vector{SVector{3,T}}, normals)
    n = length(vs)
    ns === nothing || length(ns) == n || error("assign_points: $(length(ns)) normals for $n points")
    cs = RhShape[_assign_shape(x) for x in shapes]
    b = length(cs)
    b <= 1024 || error("assign_points: $b shapes, at most 1024 in one call")
    labels = zeros(Int32, n); dist = Vector{Cdouble}(undef, n)
    counts = zeros(Int64, b + 1); offsets = zeros(Int64, b + 2); idx = Vector{Int64}(undef, n)
    np = ns === nothing ? Ptr{T}(C_NULL) : pointer(reinterpret(T, ns))
    flags = use_normals ? 0 : 1
    GC.@preserve vs ns begin
        if T == Float32
            check(ccall((:rh_assign_points_f32, LIB), Cint,
                (Ptr{Cfloat}, Ptr{Cfloat}, Int64, Ptr{RhShape}, Int32, Ref{RhParams}, Int32, Cint, Ptr{Int32}, Ptr{Cdouble},
                 Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
                pointer(reinterpret(Float32, vs)), np, n, cs, b, cparams, flags, device, labels, dist, counts, offsets, idx))
        else
            check(ccall((:rh_assign_points, LIB), Cint,
                (Ptr{Cdouble}, Ptr{Cdouble}, Int64, Ptr{RhShape}, Int32, Ref{RhParams}, Int32, Cint, Ptr{Int32}, Ptr{Cdouble},
                 Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
                pointer(reinterpret(Float64, vs)), np, n, cs, b, cparams, flags, device, labels, dist, counts, offsets, idx))
        end
    end
    return labels, dist, counts, offsets, idx
end

"""
    assign_cloud(h, shapes, params; enabled_only = false, use_normals = true) -> (labels, dist, counts, offsets, idx)

`assign_points` on the cloud's resident points (`rh_cloud_assign`; Float64 and Float32 clouds, both tested in binary64).
`enabled_only`: a disabled point gets label 0 whatever its geometry.  Nothing on the cloud changes.
"""
function assign_cloud(h::HIPCloud, shapes, params; enabled_only::Bool = false, use_normals::Bool = true, cparams = toC(params))
    n = h.pc.size
    cs = RhShape[_assign_shape(x) for x in shapes]
    b = length(cs)
    b <= 1024 || error("assign_cloud: $b shapes, at most 1024 in one call")
    labels = zeros(Int32, n); dist = Vector{Cdouble}(undef, n)
    counts = zeros(Int64, b + 1); offsets = zeros(Int64, b + 2); idx = Vector{Int64}(undef, n)
    flags = (use_normals ? 0 : 1) | (enabled_only ? 2 : 0)
    check(ccall((:rh_cloud_assign, LIB), Cint,
        (Ptr{Cvoid}, Ptr{RhShape}, Int32, Ref{RhParams}, Int32, Ptr{Int32}, Ptr{Cdouble}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
        h.handle, cs, b, cparams, flags, labels, dist, counts, offsets, idx))
    return labels, dist, counts, offsets, idx
end

end # module
