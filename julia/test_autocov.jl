# test_autocov.jl -- autocov! (julia/PixellHIP.jl, DESIGN.md 4.22) against the double loop of its definition, beside
# test_pixellhip.jl and run the same way (not run in this repository's CI: no Julia in the build image):
#     PIXELL_HIP_LIB=/path/to/libpixell_hip.so julia --project test_autocov.jl
using Test
include("PixellHIP.jl")
using .PixellHIP

@testset "autocov!: sums and pairs over the live pairs of one segment, a NaN under a cut stays out" begin
    nt, nd, lam = 300, 2, 7
    seg = Int64[10, 100, 101, 290]                                       # 0-based offsets: gaps of 10 samples at both ends
    x = randn(nt, nd)
    w = Float64.(rand(nt, nd) .>= 0.1); w[50, 2] = 0.0
    x[50, 2] = NaN
    sums, pairs = autocov!(HIPArray{Float64}(undef, lam + 1, nd), HIPArray(x), HIPArray(seg); wlive=HIPArray(w),
                           pairs=HIPArray{Int64}(undef, lam + 1, nd))
    sums, pairs = Array(sums), Array(pairs)
    sid = zeros(Int, nt)
    for s in 1:length(seg)-1
        sid[seg[s]+1:seg[s+1]] .= s
    end
    for r in 1:nd, k in 0:lam
        live = (sid .> 0) .& (w[:, r] .> 0)
        ts = [t for t in 1:nt-k if live[t] && live[t+k] && sid[t] == sid[t+k]]
        @test pairs[k+1, r] == length(ts)
        @test abs(sums[k+1, r] - sum(big(x[t, r]) * big(x[t+k, r]) for t in ts; init=big(0.0))) < 1e-11
    end
    # without wlive every sample of a segment is live; without pairs only sums comes back, the same bits
    x2 = randn(nt, nd)
    alone = Array(autocov!(HIPArray{Float64}(undef, lam + 1, nd), HIPArray(x2), HIPArray(seg)))
    both, _n = autocov!(HIPArray{Float64}(undef, lam + 1, nd), HIPArray(x2), HIPArray(seg); wlive=HIPArray(ones(nt, nd)),
                        pairs=HIPArray{Int64}(undef, lam + 1, nd))
    @test alone == Array(both)
    @test_throws Exception autocov!(HIPArray{Float64}(undef, lam + 1, nd + 1), HIPArray(x2), HIPArray(seg))
end
