# A fitted HipStandardGP without some of its observations, in O(k·N²) (include/abo_hip.h: abo_remove): the inverse of the bordered
# append.  The new model is conditioned on the remaining points in their original order, with the same hyper-parameters; `m` stays
# valid and unchanged.  A sliding window (drop the oldest point, append the newest), a discarded outlier, a re-evaluated point: none
# of them needs the O(N³) refit.  Beyond the library's crossover rule (many indices at once) the call refits the remaining points on
# the device.  Candidate sets and sample paths in sync with `m` stay with `m`.
# Single-device HipStandardGP only.  Included by HipStandardGP.jl, whose _check / _with it uses.
#
#     m2 = remove_points(m, 1)              # without the first (oldest) observation; indices are 1-based
#     m2 = remove_points(m, [3, 17, 40])

function remove_points(m::HipStandardGP, idx)
    m.gpx === nothing && throw(ArgumentError("surrogate is not conditioned on data yet (gpx === nothing)"))
    m.gpx.multi && throw(ArgumentError("remove_points runs on a single-device HipStandardGP"))
    ix = sort!(collect(Int64, idx isa Integer ? (idx,) : idx)) .- 1
    allunique(ix) || throw(ArgumentError("remove_points: an index is repeated"))
    h = Ref{Ptr{Cvoid}}(); path = Ref{Int32}(0)
    GC.@preserve ix _check(@abocall LIBABO.abo_remove(m.gpx.ptr::Ptr{Cvoid}, ix::Ptr{Int64}, Int32(length(ix))::Int32, path::Ptr{Int32},
                                                      h::Ptr{Ptr{Cvoid}})::Int32)
    _with(m, AboHandle(h[]))
end
