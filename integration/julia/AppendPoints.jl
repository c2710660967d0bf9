# A fitted HipStandardGP conditioned on k more observations in ONE blocked bordered step (include/abo_hip.h: abo_append_batch): the
# inverse of remove_points, and what a batch loop calls after it has evaluated the q points of a batch acquisition in parallel.  The
# two triangles of the factor's inverse are streamed once for all k points instead of k times, with one host wait instead of k.  The
# new model shares the factor storage of `m`, which stays valid and unchanged; when the storage has no room, or another model has
# appended past `m`, the call refits all points on the device.  Candidate sets and sample paths in sync with `m` stay with `m`.
# Single-device, value-only HipStandardGP only.  Included by HipStandardGP.jl, whose _check / _with it uses.
#
#     m2 = append_points(m, xs, ys)         # xs: a vector of k d-vectors, or a d × k matrix (one point per column); ys: k values

function append_points(m::HipStandardGP, xs, ys)
    m.gpx === nothing && throw(ArgumentError("surrogate is not conditioned on data yet (gpx === nothing)"))
    m.gpx.multi && throw(ArgumentError("append_points runs on a single-device HipStandardGP"))
    X = xs isa AbstractMatrix ? Matrix{Float64}(xs) : reduce(hcat, [collect(Float64, x) for x in xs])    # d × k: row-major k × d for C
    y = collect(Float64, ys)
    d, k = size(X)
    k >= 1 || throw(ArgumentError("append_points: the batch is empty"))
    k == length(y) || throw(DimensionMismatch("append_points: $k points but $(length(y)) targets"))
    h = Ref{Ptr{Cvoid}}(); info = Ref{Int64}(0)
    GC.@preserve X y _check(@abocall(LIBABO.abo_append_batch(m.gpx.ptr::Ptr{Cvoid}, X::Ptr{Float64}, Int32(k)::Int32, Int32(d)::Int32,
                                                             y::Ptr{Float64}, Int32(0)::Int32, info::Ptr{Int64},
                                                             h::Ptr{Ptr{Cvoid}})::Int32), info[])
    _with(m, AboHandle(h[]))
end
