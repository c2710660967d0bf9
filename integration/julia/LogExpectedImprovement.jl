# LogExpectedImprovement: log EI, evaluated on the device so that it is finite for every finite z = Δ/σ (include/abo_hip.h:
# ABO_ACQ_LOGEI = 5; Ament et al. 2023).  EI itself is exactly 0.0 from z ≈ −39 down — late in a run at N in the thousands that is most
# of a grid, every such candidate ties and `sortperm` keeps the first k grid points — and its gradient is below Optim's g_tol long
# before that, so the refinement returns every start unchanged.  LogEI has EI's arg-max and EI's order wherever EI > 0.
# Included by HipStandardGP.jl, whose _acq / _acq_args / _terms / _optimize_terms it uses: no ccall of its own.
#
#     acqf = LogExpectedImprovement(0.01, minimum(ys))          # in place of ExpectedImprovement(0.01, minimum(ys))

struct LogExpectedImprovement{Y} <: AbstractAcquisition
    ξ::Y
    best_y::Y
end
Base.copy(a::LogExpectedImprovement) = LogExpectedImprovement(a.ξ, a.best_y)
# best_y follows the data as ExpectedImprovement's does (ExpectedImprovement.jl:81-83)
update(a::LogExpectedImprovement, ys::AbstractVector, surrogate::AbstractSurrogate) =
    LogExpectedImprovement(a.ξ, _get_minimum(surrogate, ys))

_acq_args(a::LogExpectedImprovement) = (Int32(5), Float64(a.ξ), Float64(a.best_y))
(a::LogExpectedImprovement)(m::HipStandardGP, x::AbstractVector) = _acq(m, x, _acq_args(a)...)[1]

# one term of weight 1 of a weighted-sum objective; as a member of an EnsembleAcquisition it flattens like the others
_terms(a::LogExpectedImprovement, w=1.0) = (t = _acq_args(a); [AboAcqTerm(t[1], Int32(0), t[2], t[3], Float64(w))])

# grid stage + refinement in one call (abo_optimize_acquisition_terms with the single term: the bits of abo_optimize_acquisition)
function optimize_acquisition(acqf::LogExpectedImprovement, m::HipStandardGP, domain::ContinuousDomain; n_grid::Int=10_000,
                              n_local::Int=100, seed::UInt64=rand(UInt64))
    m.gpx === nothing && throw(ArgumentError("surrogate is not conditioned on data yet (gpx === nothing)"))
    _optimize_terms(_terms(acqf), m.gpx, domain, n_grid, n_local, seed)
end
