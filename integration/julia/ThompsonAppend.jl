# Sample paths that FOLLOW the model through appends (include/abo_hip.h: abo_paths_append, _attach, _detach, _top, _values,
# _append_stats_get).  Included by HipStandardGP.jl, whose HipSamplePaths / HipCandidates / @abocall / _check it uses.
#
# Per BO step, after the first `attach_paths!(p, c)`:
#     m2 = append_observation!(c, x, y)        # abo_append → abo_cand_downdate
#     append_paths!(p, m2)                      # abo_paths_append: v_s and the resident values follow, the arg-mins are left behind
#     v, idx = path_top(p)                      # abo_paths_top, k = 1: no further pass
# The advanced paths are exact posterior draws under the appended model, but they share their prior draw (omega, phase, w) with the
# paths before the append: successive steps' paths are not independent of each other.  Call sample_paths at your own cadence for
# fresh draws.

struct AboPathsAppendStats   # must match `struct abo_paths_append_stats` (include/abo_hip.h)
    model_ms::Float64; resident_ms::Float64; resident_bytes::Float64
    column_from_chain::Int64; appends::Int64
end

# advance the paths in place to m2 = append(p.model, x, y); one fresh N(0,1) draw per path joins p.eps as its last row
function append_paths!(p::HipSamplePaths, m2::HipStandardGP; eps_new::Vector{Float64}=randn(p.S))
    length(eps_new) == p.S || error("append_paths!: eps_new holds $(length(eps_new)) values, the object has S = $(p.S) paths")
    GC.@preserve eps_new _check(@abocall LIBABO.abo_paths_append(p.ptr::Ptr{Cvoid}, m2.gpx.ptr::Ptr{Cvoid}, eps_new::Ptr{Float64},
                                                                  0::Int32)::Int32)
    p.eps = vcat(p.eps, reshape(eps_new, 1, :))
    p.model = m2
    p
end

# keep g_s(z_j) of every grid point on the device (S × M doubles); the caller keeps `c` alive while it is attached
function attach_paths!(p::HipSamplePaths, c::HipCandidates)
    c.multi && error("attach_paths!: sample paths run on one device; this grid is sharded")
    _check(@abocall LIBABO.abo_paths_attach(p.ptr::Ptr{Cvoid}, c.ptr::Ptr{Cvoid})::Int32)
    p
end
detach_paths!(p::HipSamplePaths) = (_check(@abocall LIBABO.abo_paths_detach(p.ptr::Ptr{Cvoid})::Int32); p)

# per path the k attached grid points with the smallest resident g_s: (values k × S, 1-based indices k × S; 0 = no candidate)
function path_top(p::HipSamplePaths; k::Int=1)
    v = Matrix{Float64}(undef, k, p.S); idx = Matrix{Int64}(undef, k, p.S)
    GC.@preserve v idx _check(@abocall LIBABO.abo_paths_top(p.ptr::Ptr{Cvoid}, 0::Int64, Int32(k)::Int32, v::Ptr{Float64},
                                                             idx::Ptr{Int64}, 0::Int32)::Int32)
    v, idx .+ 1
end

# the resident values as an M × S matrix (column s is path s), +Inf at excluded grid points
function path_values(p::HipSamplePaths, c::HipCandidates)
    G = Matrix{Float64}(undef, c.M, p.S)
    GC.@preserve G _check(@abocall LIBABO.abo_paths_values(p.ptr::Ptr{Cvoid}, G::Ptr{Float64}, 0::Int32)::Int32)
    G
end

function append_stats(p::HipSamplePaths)
    st = Ref(AboPathsAppendStats(0.0, 0.0, 0.0, 0, 0))
    _check(@abocall LIBABO.abo_paths_append_stats_get(p.ptr::Ptr{Cvoid}, st::Ptr{AboPathsAppendStats})::Int32)
    st[]
end
