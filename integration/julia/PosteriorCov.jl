# Joint posterior covariance of a fitted HipStandardGP between point sets (include/abo_hip.h: abo_predict_cov): what AbstractGPs
# offers as cov(gpx(xa)), cov(gpx(xa), gpx(xb)) and mean_and_cov(gpx(x)) — the latent covariance, no observation noise, computed on the
# device from the resident L⁻¹ (no N² read-back).  The symmetric form is symmetric bit for bit and carries the FiniteGP jitter 1e-18 on
# its diagonal, as posterior_var does.  1 to 8192 points per set.  With it a caller scores a batch of its own jointly (q-EI of given
# points, P(f(a) < f(b))) or draws exact joint samples: μ .+ cholesky(Symmetric(Σ + ϵI)).L * randn(M).
# Single-device HipStandardGP only.  Included by HipStandardGP.jl, whose _check / _pack it uses.
#
#     Σ = posterior_cov(model, xa)            # Ma × Ma
#     Σ = posterior_cov(model, xa, xb)        # Ma × Mb
#     μ, Σ = mean_and_cov(model, xa)

function _cov_handle(m::HipStandardGP)
    m.gpx === nothing && throw(ArgumentError("surrogate is not conditioned on data yet (gpx === nothing)"))
    m.gpx.multi && throw(ArgumentError("posterior_cov runs on a single-device HipStandardGP"))
    m.gpx.ptr
end

function posterior_cov(m::HipStandardGP, xa::AbstractVector)
    h = _cov_handle(m); Z = _pack(xa); d, M = size(Z)
    Σ = Matrix{Float64}(undef, M, M)
    GC.@preserve Z Σ _check(@abocall LIBABO.abo_predict_cov(h::Ptr{Cvoid}, Z::Ptr{Float64}, M::Int64, C_NULL::Ptr{Float64}, 0::Int64,
        d::Int32, 0::Int32, C_NULL::Ptr{Float64}, C_NULL::Ptr{Float64}, Σ::Ptr{Float64}, 0::Int32)::Int32)
    Σ
end

# the library writes row-major Ma × Mb: read column-major that is the transpose
function posterior_cov(m::HipStandardGP, xa::AbstractVector, xb::AbstractVector)
    h = _cov_handle(m); Za = _pack(xa); Zb = _pack(xb); d, Ma = size(Za); db, Mb = size(Zb)
    d == db || throw(DimensionMismatch("xa has dimension $d, xb has dimension $db"))
    Σt = Matrix{Float64}(undef, Mb, Ma)
    GC.@preserve Za Zb Σt _check(@abocall LIBABO.abo_predict_cov(h::Ptr{Cvoid}, Za::Ptr{Float64}, Ma::Int64, Zb::Ptr{Float64}, Mb::Int64,
        d::Int32, 0::Int32, C_NULL::Ptr{Float64}, C_NULL::Ptr{Float64}, Σt::Ptr{Float64}, 0::Int32)::Int32)
    permutedims(Σt)
end

function mean_and_cov(m::HipStandardGP, xa::AbstractVector)
    h = _cov_handle(m); Z = _pack(xa); d, M = size(Z)
    μ = Vector{Float64}(undef, M); Σ = Matrix{Float64}(undef, M, M)
    GC.@preserve Z μ Σ _check(@abocall LIBABO.abo_predict_cov(h::Ptr{Cvoid}, Z::Ptr{Float64}, M::Int64, C_NULL::Ptr{Float64}, 0::Int64,
        d::Int32, 0::Int32, μ::Ptr{Float64}, C_NULL::Ptr{Float64}, Σ::Ptr{Float64}, 0::Int32)::Int32)
    μ, Σ
end
