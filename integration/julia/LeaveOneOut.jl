# Leave-one-out cross-validation of a fitted HipStandardGP (include/abo_hip.h: abo_loo, abo_loo_grad; Rasmussen & Williams §5.4.2): the
# predictive mean and variance of every observed target when that target is left out (noise included), its log predictive density, and
# nlpl = −Σ lpd — from the model's resident L⁻¹ in one pass, no refit.  Standardised residuals (ys .- μ) ./ sqrt.(σ²) flag outliers and a
# wrong noise level; nlpl is the alternative hyper-parameter objective when NLML over-fits a misspecified kernel family.
# Single-device HipStandardGP only.  Included by HipStandardGP.jl, whose _check / _fitted_with it uses.
#
#     μ, σ², lpd, nlpl = leave_one_out(model)
#     v, g = loo_and_grad(model, [log ℓ, log σ_f²], xs, ys)

function _loo_handle(m::HipStandardGP)
    m.gpx === nothing && throw(ArgumentError("surrogate is not conditioned on data yet (gpx === nothing)"))
    m.gpx.multi && throw(ArgumentError("leave_one_out runs on a single-device HipStandardGP"))
    m.gpx.ptr
end

function leave_one_out(m::HipStandardGP)
    h = _loo_handle(m); n = Ref{Int64}(); d = Ref{Int32}()
    _check(@ccall LIBABO.abo_get_n(h::Ptr{Cvoid}, n::Ptr{Int64}, d::Ptr{Int32})::Int32)
    μ = Vector{Float64}(undef, n[]); σ² = Vector{Float64}(undef, n[]); lpd = Vector{Float64}(undef, n[]); v = Ref{Float64}()
    GC.@preserve μ σ² lpd _check(@ccall LIBABO.abo_loo(h::Ptr{Cvoid}, μ::Ptr{Float64}, σ²::Ptr{Float64}, lpd::Ptr{Float64},
                                                       v::Ptr{Float64}, 0::Int32)::Int32)
    μ, σ², lpd, v[]
end

# value and analytic gradient w.r.t. (log ℓ, log σ_f²) from ONE refit, the parameter convention of nlml_and_grad
function loo_and_grad(m::HipStandardGP, params, xs::AbstractVector, ys::AbstractVector)
    v = Ref{Float64}(); g1 = Ref{Float64}(); g2 = Ref{Float64}(); f = _fitted_with(m, params[1], params[2], xs, ys)
    _check(@ccall LIBABO.abo_loo_grad(_loo_handle(f)::Ptr{Cvoid}, v::Ptr{Float64}, g1::Ptr{Float64}, g2::Ptr{Float64},
                                      C_NULL::Ptr{Float64})::Int32)
    v[], [g1[], g2[]]
end
