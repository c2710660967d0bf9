# MaxValueEntropySearch: max-value entropy search (include/abo_hip.h: ABO_ACQ_MES = 6; Wang & Jegelka 2017), the information-theoretic
# acquisition that is cheap enough for a 2²⁰-point grid: the mean over S samples y* of the objective's minimum value of
# a(γ) = γ·φ(γ)/(2Φ(γ)) − log Φ(γ), γ = (μ − y*)/σ.  Nothing to tune; the samples are the minima of Thompson sample paths over a grid
# (max_value_samples below: path_argmin with k = 1).  Its parameter is a vector, so it has entry points of its own (abo_*_mes) instead
# of the (kind, p0, best_y) triple, and it is no member of an EnsembleAcquisition.  Single-device HipStandardGP only.
# Included by HipStandardGP.jl, whose _pack / _check / @abocall / sample_paths / path_argmin it uses.
#
#     ystar = max_value_samples(model, grid, 16)
#     acqf  = MaxValueEntropySearch(ystar)
#     x     = optimize_acquisition(acqf, model, domain)

struct MaxValueEntropySearch <: AbstractAcquisition
    ystar::Vector{Float64}
    function MaxValueEntropySearch(ystar::AbstractVector{<:Real})
        1 <= length(ystar) <= 1024 || throw(ArgumentError("MaxValueEntropySearch takes 1 to 1024 samples, got $(length(ystar))"))
        all(isfinite, ystar) || throw(ArgumentError("MaxValueEntropySearch: the samples must be finite"))
        new(collect(Float64, ystar))
    end
end
Base.copy(a::MaxValueEntropySearch) = MaxValueEntropySearch(copy(a.ystar))
# new data calls for new samples: the caller draws them (max_value_samples) and builds a new object
update(a::MaxValueEntropySearch, ys::AbstractVector, surrogate::AbstractSurrogate) = a

# S samples of the minimum value: each path's minimum over the grid (or a resident candidate set)
function max_value_samples(m::HipStandardGP, zs_or_cands, S::Int; R::Int=1024, rng=Random.default_rng())
    v, _ = path_argmin(sample_paths(m, S; R=R, rng=rng), zs_or_cands; k=1)
    vec(v)
end

function _mes_handle(m::HipStandardGP)
    m.gpx === nothing && throw(ArgumentError("surrogate is not conditioned on data yet (gpx === nothing)"))
    m.gpx.multi && throw(ArgumentError("MaxValueEntropySearch runs on a single-device HipStandardGP"))
    m.gpx.ptr
end

# scores and, for k > 0, the first k of sortperm(scores; rev=true) (1-based), as _acq returns them
function _acq_mes(m::HipStandardGP, x, a::MaxValueEntropySearch; k=0, scores=true)
    h = _mes_handle(m); Z = _pack(x); d, M = size(Z); ys = a.ystar; S = length(ys)
    s = scores ? Vector{Float64}(undef, M) : Float64[]; ps = scores ? pointer(s) : Ptr{Float64}(C_NULL)
    tv = Vector{Float64}(undef, k); ti = Vector{Int64}(undef, k)
    GC.@preserve Z ys s tv ti _check(@abocall LIBABO.abo_acq_mes(h::Ptr{Cvoid}, Z::Ptr{Float64}, M::Int64, d::Int32, 0::Int32,
        ys::Ptr{Float64}, S::Int32, 0::Int32, 0::Int64, ps::Ptr{Float64}, k::Int32, tv::Ptr{Float64}, ti::Ptr{Int64}, 0::Int32)::Int32)
    s, tv, ti .+ 1
end
(a::MaxValueEntropySearch)(m::HipStandardGP, x::AbstractVector) = _acq_mes(m, x, a)[1]

# no member of a weighted sum: abo_acq_term has no room for the samples
_terms(a::MaxValueEntropySearch, w=1.0) =
    throw(ArgumentError("MaxValueEntropySearch cannot be a member of an EnsembleAcquisition; evaluate it on its own"))

# grid stage + refinement in one call
function optimize_acquisition(acqf::MaxValueEntropySearch, m::HipStandardGP, domain::ContinuousDomain; n_grid::Int=10_000,
                              n_local::Int=100, seed::UInt64=rand(UInt64))
    h = _mes_handle(m); ys = acqf.ystar; S = length(ys)
    lower = collect(Float64, domain.lower); upper = collect(Float64, domain.upper); d = length(lower)
    bx = Vector{Float64}(undef, d); bv = Ref{Float64}(); opts = Ref(AboRefineOpts(0, 0, 0, 0, 0.0, 0.0, 0.0))
    GC.@preserve ys lower upper bx _check(@abocall LIBABO.abo_optimize_acquisition_mes(h::Ptr{Cvoid}, ys::Ptr{Float64}, S::Int32,
        lower::Ptr{Float64}, upper::Ptr{Float64}, d::Int32, n_grid::Int64, n_local::Int32, seed::UInt64, opts::Ptr{AboRefineOpts},
        bx::Ptr{Float64}, bv::Ptr{Float64}, C_NULL::Ptr{Float64}, C_NULL::Ptr{Float64}, C_NULL::Ptr{Float64},
        C_NULL::Ptr{Float64})::Int32)
    bx
end
