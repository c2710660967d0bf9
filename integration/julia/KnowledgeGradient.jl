# Knowledge gradient of a fitted HipStandardGP over a discrete decision set (include/abo_hip.h: abo_acq_kg): the expected decrease of the
# minimum of the posterior mean over the decision set from one observation at a candidate (Frazier, Powell and Dayanik 2009; with the
# candidate's own point added, the KGCP of Scott et al. 2011).  It needs no best_y and no ξ or β, which is what a noisy objective calls
# for.  The joint covariance between candidates and decision set stays on the device: one number per candidate comes back.
# 1 to 8192 points per set.  Single-device HipStandardGP only.  Included by HipStandardGP.jl, whose _check / _pack it uses.
#
#     s = knowledge_gradient(model, xs)                      # the decision set is xs itself
#     s = knowledge_gradient(model, xs, decision)            # … a given set, each candidate's own point added (include_self = true)
#     s, vals, idx = knowledge_gradient(model, xs, decision; k = 10)     # idx 1-based, descending, ties to the lowest index

const ABO_KG_SELF = Int32(1)

function _kg_handle(m::HipStandardGP)
    m.gpx === nothing && throw(ArgumentError("surrogate is not conditioned on data yet (gpx === nothing)"))
    m.gpx.multi && throw(ArgumentError("knowledge_gradient runs on a single-device HipStandardGP"))
    m.gpx.ptr
end

# noise === nothing: the noise the factor was built with (a negative value at the C-ABI)
function knowledge_gradient(m::HipStandardGP, xs::AbstractVector, decision::Union{Nothing,AbstractVector}=nothing;
                            noise::Union{Nothing,Real}=nothing, include_self::Bool=true, k::Integer=0)
    h = _kg_handle(m); Za = _pack(xs); d, Ma = size(Za)
    Zb = decision === nothing ? nothing : _pack(decision)
    Mb = Zb === nothing ? 0 : size(Zb, 2)
    Zb === nothing || size(Zb, 1) == d || throw(DimensionMismatch("xs has dimension $d, decision has dimension $(size(Zb, 1))"))
    zb = Zb === nothing ? Ptr{Float64}(C_NULL) : pointer(Zb)
    flags = (Zb !== nothing && include_self) ? ABO_KG_SELF : Int32(0)
    nz = noise === nothing ? -1.0 : Float64(noise)
    s = Vector{Float64}(undef, Ma); tv = Vector{Float64}(undef, max(k, 1)); ti = Vector{Int64}(undef, max(k, 1))
    GC.@preserve Za Zb s tv ti _check(@abocall LIBABO.abo_acq_kg(h::Ptr{Cvoid}, Za::Ptr{Float64}, Ma::Int64, zb::Ptr{Float64}, Mb::Int64,
        d::Int32, 0::Int32, nz::Float64, flags::Int32, 1::Int64, s::Ptr{Float64}, k::Int32, tv::Ptr{Float64}, ti::Ptr{Int64}, 0::Int32)::Int32)
    k == 0 ? s : (s, tv[1:k], ti[1:k])
end
