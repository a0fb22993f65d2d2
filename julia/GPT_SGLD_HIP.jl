# GPT_SGLD_HIP — drop-in replacement of the reference's `GPT_SGLD` module entry points on the
# MI355X path, via `ccall` into libgptsgld.so (include/gptsgld.h).  Julia is not on the image:
# tests/test_julia_shim.py checks every ccall against the C prototypes, and the Python binding
# gpt_amd/GPT_SGLD.py (tested on the GPU) makes the identical C calls.
#
#   kin40kExperiment.jl:  `@everywhere using GPT_SGLD`  ->  `@everywhere using GPT_SGLD_HIP`
#
# Arrays are passed zero-copy (Julia column-major == the C ABI layout); outputs are allocated here,
# exactly as the reference functions allocate and return them.
module GPT_SGLD_HIP

export datawhitening, feature, feature_inputs, featureNotensor, samplenz, GPTregression, GPTregression_chains,
       GPTregression_chains_x, GPT_SGLDERM, pred, RMSE,
       GPNT_SGLD, GPNT_SGLD_chains, GPNT_SGLD_chains_x, GPNT_pred, GPNT_pred_x, GPT_SGLDERM_RMSprop, GPT_SGLDERMw, GPTclassification, GPT_GMC, pred_mean_x,
       init_state, GPNT_nlogmarginal, GPNT_gradnlogmarginal, GP_nlogmarginal, GP_gradnlogmarginal, GP_predict, GPNT_predict, RFF_kernel_error,
       GPNT_SGLDclass, GPNT_SGLDclass_chains, class_eval, GPNT_pred_class, pred_class,
       neglogjointlkhd, gradneglogjointlkhd, joint_langevin, joint_scores, joint_hmc, joint_mala,
       predictive, pred_predictive, pred_predictive_x, GPNT_predictive, GPNT_predictive_x,
       chain_diagnostics,
       GPrand, GPpost_rand, GPNT_draw_theta, fhatdraw, createmesh

const LIB = get(ENV, "GPTSGLD_LIB", joinpath(@__DIR__, "..", "gpt_amd", "libgptsgld.so"))

struct SGLDConfig          # gpt_sgld_config
    n::Int64; D::Int64; N::Int64; r::Int64; Q::Int64; m::Int64
    epsw::Float64; epsU::Float64; signal_var::Float64; sigma_w::Float64
    burnin::Int64; maxepoch::Int64; seed::UInt64
    langevin::Int32; stiefel::Int32; store_every::Int64; max_steps::Int64
end

lasterr() = unsafe_string(ccall((:gpt_last_error, LIB), Cstring, ()))
check(rc) = rc == 0 ? nothing : error("gptsgld error $rc: " * lasterr())

# GPT_SGLD.jl:62-67 (host data prep, unchanged semantics)
function datawhitening(X::Array)
    X = copy(X)
    for i = 1:size(X, 2)
        X[:, i] = (X[:, i] .- sum(X[:, i]) / size(X, 1)) ./ sqrt(sum(abs2, X[:, i] .- sum(X[:, i]) / size(X, 1)) / (size(X, 1) - 1))
    end
    return X
end

# feature(X,length_scale,sigma_RBF,phi_scale,Z,b)  GPT_SGLD.jl:71
function feature(X::Array{Float64,2}, length_scale, sigma_RBF::Real, phi_scale::Real,
                 Z::Array{Float64,2}, b::Array{Float64})
    N, D = size(X); n = size(Z, 1)
    ls = collect(Float64, length_scale isa Real ? [length_scale] : length_scale)
    phi = Array{Float64}(undef, n, D, N)
    check(ccall((:gpt_feature, LIB), Cint,
                (Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Float64, Float64, Ptr{Float64},
                 Ptr{Float64}, Int64, Ptr{Float64}),
                X, N, D, ls, length(ls), sigma_RBF, phi_scale, Z, b, n, phi))
    return phi
end

# Generation-C seeded form used by kin40kExperiment.jl:71: feature(X,n,ls,σ,seed,scale)
function feature(X::Array{Float64,2}, n::Integer, length_scale, sigma_RBF::Real, seed::Integer,
                 scale::Real)
    D = size(X, 2)
    Z = Array{Float64}(undef, n, D); b = Array{Float64}(undef, n, D)
    check(ccall((:gpt_feature_inputs, LIB), Cint, (Int64, Int64, UInt64, Ptr{Float64}, Ptr{Float64}),
                n, D, seed, Z, b))
    return feature(X, length_scale, sigma_RBF, scale, Z, b)
end

# The Z = randn(n,D), b = 2π·rand(n,D) that the seeded form above draws, for the entry points that
# take X, Z and b in place of a phi (GPTregression_chains_x, pred_mean_x)
function feature_inputs(n::Integer, D::Integer, seed::Integer)
    Z = Array{Float64}(undef, n, D); b = Array{Float64}(undef, n, D)
    check(ccall((:gpt_feature_inputs, LIB), Cint, (Int64, Int64, UInt64, Ptr{Float64}, Ptr{Float64}),
                n, D, seed, Z, b))
    return Z, b
end

# Generation-A seeded form feature(X,n,length_scale,seed) (GPT_SGLD_p.jl:40-54): Z = randn(n,D)
# / length_scale, b = randn(n,D), phi = sqrt(2/n)·cos(X[i,k]·Z[j,k] + b[j,k]) — no sigma_RBF, no
# scale (gpt_feature_inputs_a draws Z and b on the framework's Philox contract)
function feature(X::Array{Float64,2}, n::Integer, length_scale::Real, seed::Integer)
    D = size(X, 2)
    Z = Array{Float64}(undef, n, D); b = Array{Float64}(undef, n, D)
    check(ccall((:gpt_feature_inputs_a, LIB), Cint, (Int64, Int64, UInt64, Ptr{Float64}, Ptr{Float64}),
                n, D, seed, Z, b))
    return feature(X, 1.0, 1.0, 1.0, Z ./ length_scale, b)
end

# featureNotensor(X,length_scale,sigma_RBF,Z,b)  GPT_SGLD.jl:109
function featureNotensor(X::Array{Float64,2}, length_scale, sigma_RBF::Real, Z::Array{Float64,2},
                         b::Array{Float64})
    N, D = size(X); n = size(Z, 1)
    ls = collect(Float64, length_scale isa Real ? [length_scale] : length_scale)
    phi = Array{Float64}(undef, n, N)
    check(ccall((:gpt_feature_notensor, LIB), Cint,
                (Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Float64, Ptr{Float64},
                 Ptr{Float64}, Int64, Ptr{Float64}),
                X, N, D, ls, length(ls), sigma_RBF, Z, b, n, phi))
    return phi
end

# Generation-C seeded form featureNotensor(X,n,length_scale,sigma_RBF,seed), the call of
# PowerPlantNoTensorExperiment.jl:32-33, kin40kNoTensorExperiment.jl:35-36 and
# PowerPlantDataExperiment.jl:159: Z = randn(n,D), b = 2π·rand(n) drawn by gpt_feature_inputs on
# the framework's Philox contract (column 1 of its b), then the Gen-D map above
function featureNotensor(X::Array{Float64,2}, n::Integer, length_scale, sigma_RBF::Real,
                         seed::Integer)
    D = size(X, 2)
    Z = Array{Float64}(undef, n, D); b = Array{Float64}(undef, n, D)
    check(ccall((:gpt_feature_inputs, LIB), Cint, (Int64, Int64, UInt64, Ptr{Float64}, Ptr{Float64}),
                n, D, seed, Z, b))
    return featureNotensor(X, length_scale, sigma_RBF, Z, b[:, 1])
end

# samplenz(r,D,Q,seed)  GPT_SGLD_p.jl:57
function samplenz(r::Integer, D::Integer, Q::Integer, seed::Integer=0)
    I = Array{Int32}(undef, Q, D)
    check(ccall((:gpt_samplenz, LIB), Cint, (Int64, Int64, Int64, UInt64, Ptr{Int32}), r, D, Q, seed, I))
    return I
end

# GPTregression(phi,y,signal_var,I,r,Q,m,epsw,epsU,burnin,maxepoch,param_seed;langevin,stiefel)
# GPT_SGLD.jl:345 — returns (w_store, U_store); NaN in the geodesic -> message + zeros (:422-424).
function GPTregression(phi::Array{Float64,3}, y::Array{Float64}, signal_var::Real, I::Array{Int32,2},
                       r::Integer, Q::Integer, m::Integer, epsw::Real, epsU::Real, burnin::Integer,
                       maxepoch::Integer, param_seed::Integer=0; langevin=true, stiefel=true,
                       sigma_w::Real=1.0, store_every::Integer=1)
    n, D, N = size(phi)
    numbatches = cld(N, m)
    T = div(maxepoch * numbatches, store_every)
    cfg = Ref(SGLDConfig(n, D, N, r, Q, m, epsw, epsU, signal_var, sigma_w, burnin, maxepoch,
                         UInt64(param_seed), Int32(langevin), Int32(stiefel), store_every, 0))
    w_store = zeros(Q, T); U_store = zeros(n, r, D, T)
    rc = ccall((:gpt_sgld_regression, LIB), Cint,
               (Ref{SGLDConfig}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64},
                Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
               cfg, phi, vec(y), I, C_NULL, C_NULL, w_store, U_store, C_NULL)
    if rc == 1
        println("Get NaN when moving along Geodesic. Try smaller epsU")
        return zeros(Q, T), zeros(n, r, D, T)
    end
    check(rc)
    return w_store, U_store
end

# The sweep block of kin40kExperiment.jl:67-74 (`@parallel for j=1:10`, one GPTregression per sweep
# on that sweep's phitrain) as one call: chain j runs on phis[j] with param_seeds[j] (epsw, epsU,
# signal_var: one value, or one per chain) in one device session (gpt_sgld_regression_chains: the
# chain engine at r <= 5, the wave engine at kin40k's r = 20).  Returns [(w_store, U_store, status)]
# per chain; status 1 = the geodesic NaN bail-out (message + zero stores, :422-424).
function GPTregression_chains(phis::Vector{Array{Float64,3}}, y::Array{Float64}, signal_var,
                              I::Array{Int32,2}, r::Integer, Q::Integer, m::Integer, epsw, epsU,
                              burnin::Integer, maxepoch::Integer, param_seeds::Vector{<:Integer};
                              sigma_w::Real=1.0, store_every::Integer=1)
    C = length(param_seeds)
    C >= 1 || error("need at least one chain")
    length(phis) == C || error("one phi per chain")
    n, D, N = size(phis[1])
    # the library reads n*D*N doubles of every phi, N of y, Q*D of I and C of every per-chain vector
    all(p -> size(p) == (n, D, N), phis) || error("every phi must have the same (n, D, N)")
    length(y) == N || error("phi and y disagree on N")
    size(I) == (Q, D) || error("I must be (Q, D)")
    T = div(maxepoch * cld(N, m), store_every)
    perchain(v) = v isa Real ? fill(Float64(v), C) : collect(Float64, v)
    ew, eu, sv = perchain(epsw), perchain(epsU), perchain(signal_var)
    length(ew) == C && length(eu) == C && length(sv) == C ||
        error("epsw, epsU and signal_var: one value, or one per chain")
    cfg = Ref(SGLDConfig(n, D, N, r, Q, m, ew[1], eu[1], sv[1], sigma_w, burnin, maxepoch,
                         UInt64(0), Int32(1), Int32(1), store_every, 0))
    ws = [zeros(Q, T) for c = 1:C]; Us = [zeros(n, r, D, T) for c = 1:C]
    yv = vec(y); status = zeros(Int32, C); seeds = UInt64.(param_seeds)
    GC.@preserve phis yv ws Us begin
        check(ccall((:gpt_sgld_regression_chains, LIB), Cint,
                    (Ref{SGLDConfig}, Int32, Ptr{UInt64}, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}},
                     Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Ptr{Float64}},
                     Ptr{Ptr{Float64}}, Ptr{Int32}),
                    cfg, Int32(C), seeds, pointer.(phis), fill(pointer(yv), C), I, ew, eu, sv,
                    pointer.(ws), pointer.(Us), status))
    end
    for c = 1:C
        status[c] == 1 && println("Get NaN when moving along Geodesic. Try smaller epsU")
    end
    return [(ws[c], Us[c], Int(status[c])) for c = 1:C]
end

# GPTregression_chains from X: the same sweep block without a phi per sweep.  Chain j trains on
# feature(X, length_scales[:,j], sigma_RBFs[j], phi_scale, Z, b), which the library forms on the
# device one minibatch ahead of the steps (gpt_sgld_regression_chains_x; the same doubles, so the
# same stores as GPTregression_chains on those phis): the host computes, holds and uploads X, Z, b
# and ls_len + 1 hyper-parameters per sweep instead of n*D*N doubles per sweep.
# length_scales: (ls_len, C) with ls_len 1 or D (a Vector of C scalars is taken as (1, C)).
function GPTregression_chains_x(X::Array{Float64,2}, y::Array{Float64}, length_scales,
                                sigma_RBFs, phi_scale::Real, Z::Array{Float64,2},
                                b::Array{Float64}, signal_var, I::Array{Int32,2}, r::Integer,
                                Q::Integer, m::Integer, epsw, epsU, burnin::Integer,
                                maxepoch::Integer, param_seeds::Vector{<:Integer};
                                sigma_w::Real=1.0, store_every::Integer=1)
    C = length(param_seeds)
    C >= 1 || error("need at least one chain")
    N, D = size(X); n = size(Z, 1)
    ls = length_scales isa AbstractVector ? reshape(collect(Float64, length_scales), 1, :) :
                                            collect(Float64, length_scales)
    ls_len = size(ls, 1)
    # the library reads N*D of X, n*D of Z and b, N of y, Q*D of I, ls_len*C length scales and C
    # of every per-chain vector
    (ls_len == 1 || ls_len == D) || error("dimensions of X and length_scale do not match")
    size(ls, 2) == C || error("one column of length scales per chain")
    size(Z) == (n, D) || error("Z must be (n, D)")
    length(b) == n * D || error("b must be (n, D)")
    length(y) == N || error("X and y disagree on N")
    size(I) == (Q, D) || error("I must be (Q, D)")
    perchain(v) = v isa Real ? fill(Float64(v), C) : collect(Float64, v)
    sg, ew, eu, sv = perchain(sigma_RBFs), perchain(epsw), perchain(epsU), perchain(signal_var)
    length(sg) == C && length(ew) == C && length(eu) == C && length(sv) == C ||
        error("sigma_RBFs, epsw, epsU and signal_var: one value, or one per chain")
    T = div(maxepoch * cld(N, m), store_every)
    cfg = Ref(SGLDConfig(n, D, N, r, Q, m, ew[1], eu[1], sv[1], sigma_w, burnin, maxepoch,
                         UInt64(0), Int32(1), Int32(1), store_every, 0))
    ws = [zeros(Q, T) for c = 1:C]; Us = [zeros(n, r, D, T) for c = 1:C]
    yv = vec(y); status = zeros(Int32, C); seeds = UInt64.(param_seeds)
    GC.@preserve yv ws Us begin
        check(ccall((:gpt_sgld_regression_chains_x, LIB), Cint,
                    (Ref{SGLDConfig}, Int32, Ptr{UInt64}, Ptr{Float64}, Ptr{Ptr{Float64}},
                     Ptr{Float64}, Int64, Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Float64},
                     Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Ptr{Float64}},
                     Ptr{Ptr{Float64}}, Ptr{Int32}),
                    cfg, Int32(C), seeds, X, fill(pointer(yv), C), ls, ls_len, sg, phi_scale, Z, b,
                    I, ew, eu, sv, pointer.(ws), pointer.(Us), status))
    end
    for c = 1:C
        status[c] == 1 && println("Get NaN when moving along Geodesic. Try smaller epsU")
    end
    return [(ws[c], Us[c], Int(status[c])) for c = 1:C]
end

# GPT_SGLDERM(phi,y,sigma,I,r,Q,m,epsw,epsU,burnin,maxepoch)  GPT_SGLD_p.jl:146 (σ_w=√(nᴰ/Q))
function GPT_SGLDERM(phi::Array{Float64,3}, y::Array{Float64}, sigma::Real, I::Array{Int32,2},
                     r::Integer, Q::Integer, m::Integer, epsw::Real, epsU::Real, burnin::Integer,
                     maxepoch::Integer, param_seed::Integer=0)
    n, D, _ = size(phi)
    return GPTregression(phi, y, sigma^2, I, r, Q, m, epsw, epsU, burnin, maxepoch, param_seed;
                         sigma_w=sqrt(Float64(n)^D / Q))
end

# GPT_SGLDERM_RMSprop(phi,y,signal_var,I,r,Q,m,epsilon,alpha,burnin,maxepoch)  GPT_SGLD.jl:1121
function GPT_SGLDERM_RMSprop(phi::Array{Float64,3}, y::Array{Float64}, signal_var::Real,
                             I::Array{Int32,2}, r::Integer, Q::Integer, m::Integer, epsilon::Real,
                             alpha::Real, burnin::Integer, maxepoch::Integer, param_seed::Integer=0)
    n, D, N = size(phi)
    T = maxepoch * cld(N, m)
    cfg = Ref(SGLDConfig(n, D, N, r, Q, m, epsilon, epsilon, signal_var, 1.0, burnin, maxepoch,
                         UInt64(param_seed), Int32(1), Int32(1), 1, 0))
    w_store = zeros(Q, T); U_store = zeros(n, r, D, T)
    rc = ccall((:gpt_sgld_rmsprop, LIB), Cint,
               (Ref{SGLDConfig}, Float64, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Int32},
                Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
               cfg, epsilon, alpha, phi, vec(y), I, C_NULL, C_NULL, w_store, U_store, C_NULL)
    if rc == 1
        return zeros(Q, T), zeros(n, r, D, T)
    end
    check(rc)
    return w_store, U_store
end

# pred(w,U,I,phitest)  GPT_SGLD.jl:233
# GPT_SGLD.jl:1065-1118 (w-only SGLD, U fixed at its Stiefel draw)
function GPT_SGLDERMw(phi::Array{Float64,3}, y::Array{Float64}, signal_var::Real, I::Array{Int32,2},
                      r::Integer, Q::Integer, m::Integer, epsw::Real, burnin::Integer, maxepoch::Integer,
                      param_seed::Integer=0)
    n, D, N = size(phi)
    cfg = SGLDConfig(n, D, N, r, Q, m, epsw, 0.0, signal_var, 1.0, burnin, maxepoch, param_seed, 1, 1, 1, 0)
    w_store = Array{Float64}(undef, Q, maxepoch * cld(N, m))
    U = Array{Float64}(undef, n, r, D)
    check(ccall((:gpt_sgld_wonly, LIB), Cint,
                (Ref{SGLDConfig}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                cfg, phi, vec(y), I, C_NULL, C_NULL, w_store, U, C_NULL))
    return w_store, U
end

# GPT_SGLD.jl:452-680 (labels y in 1..C)
function GPTclassification(phi::Array{Float64,3}, y::Array, I::Array{Int32,2}, r::Integer, Q::Integer,
                           m::Integer, epsw::Real, epsU::Real, burnin::Integer, maxepoch::Integer,
                           param_seed::Integer; langevin=true, stiefel=true)
    n, D, N = size(phi)
    C = Int(maximum(y) - minimum(y) + 1)
    cfg = SGLDConfig(n, D, N, r, Q, m, epsw, epsU, 1.0, 1.0, burnin, maxepoch, param_seed,
                     Int32(langevin), Int32(stiefel), 1, 0)
    T = maxepoch * cld(N, m)
    w_store = Array{Float64}(undef, Q, C, T); U_store = Array{Float64}(undef, n, r, D, C, T)
    rc = ccall((:gpt_sgld_classification, LIB), Cint,
               (Ref{SGLDConfig}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64},
                Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
               cfg, phi, Float64.(vec(y)), I, C_NULL, C_NULL, w_store, U_store, C_NULL)
    if rc == 1
        println("Get NaN when moving along Geodesic. Try smaller epsU")
        return zeros(Q, C, T), zeros(n, r, D, C, T)
    end
    check(rc)
    return w_store, U_store
end

# GPT_SGLD.jl:684-805 (geodesic Monte Carlo)
function GPT_GMC(phi::Array{Float64,3}, y::Array{Float64}, signal_var::Real, I::Array{Int32,2},
                 r::Integer, Q::Integer, epsw::Real, epsU::Real, burnin::Integer, maxepoch::Integer,
                 L::Integer, param_seed::Integer)
    n, D, N = size(phi)
    w_store = Array{Float64}(undef, Q, maxepoch); U_store = Array{Float64}(undef, n, r, D, maxepoch)
    accept_prob = Array{Float64}(undef, maxepoch + burnin)
    rc = ccall((:gpt_gmc, LIB), Cint,
               (Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Int64, Int64, Ptr{Int32}, Float64,
                Float64, Float64, Int64, Int64, Int64, UInt64, Ptr{Float64}, Ptr{Float64},
                Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
               phi, vec(y), n, D, N, r, Q, I, signal_var, epsw, epsU, burnin, maxepoch, L, param_seed,
               C_NULL, C_NULL, w_store, U_store, accept_prob)
    rc == 1 && println("Get NaN when moving along Geodesic. Try smaller epsU")
    rc in (0, 1) || check(rc)
    return w_store, U_store, accept_prob
end

function pred(w::Array{Float64}, U::Array{Float64,3}, I::Array{Int32,2}, phitest::Array{Float64,3})
    n, D, Nt = size(phitest); r = size(U, 2); Q = length(w)
    f = Array{Float64}(undef, Nt)
    check(ccall((:gpt_pred, LIB), Cint,
                (Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Int64, Int64, Int64, Int64, Int64,
                 Ptr{Float64}), vec(w), U, I, phitest, n, D, Nt, r, Q, f))
    return f
end

# RMSE(w_store,U_store,I,phitest,ytest)  GPT_SGLD_p.jl:124 — mean prediction over all samples
function RMSE(w_store::Array{Float64,2}, U_store::Array{Float64,4}, I::Array{Int32,2},
              phitest::Array{Float64,3}, ytest::Array{Float64})
    n, D, Nt = size(phitest); r = size(U_store, 2); Q, S = size(w_store)
    meanf = Array{Float64}(undef, Nt); out = Ref(0.0)
    check(ccall((:gpt_pred_mean, LIB), Cint,
                (Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64,
                 Int64, Int64, Int64, Float64, Ptr{Float64}, Ref{Float64}),
                w_store, U_store, I, phitest, vec(ytest), n, D, Nt, r, Q, S, 1.0, meanf, out))
    return out[]
end

# The per-epoch evaluation of kin40kExperiment.jl:78-87 with the test features formed inside the
# prediction kernel (no n·D·Ntest phitest array): returns (meanfhat, scale·RMSE of the mean,
# per-sample scale·RMSE = the testRMSE curve when the samples are the epoch ends)
function pred_mean_x(w_store::Array{Float64,2}, U_store::Array{Float64,4}, I::Array{Int32,2},
                     Xtest::Array{Float64,2}, ytest::Array{Float64}, length_scale,
                     sigma_RBF::Real, phi_scale::Real, Z::Array{Float64,2}, b::Array{Float64};
                     scale::Real=1.0)
    Nt, D = size(Xtest); n = size(Z, 1); r = size(U_store, 2); Q, S = size(w_store)
    ls = collect(Float64, length_scale isa Real ? [length_scale] : length_scale)
    meanf = Array{Float64}(undef, Nt); out = Ref(0.0); curve = Array{Float64}(undef, S)
    check(ccall((:gpt_pred_mean_x, LIB), Cint,
                (Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Int64, Int64,
                 Ptr{Float64}, Int64, Float64, Float64, Ptr{Float64}, Ptr{Float64}, Int64, Int64,
                 Int64, Int64, Float64, Ptr{Float64}, Ref{Float64}, Ptr{Float64}),
                w_store, U_store, I, Xtest, vec(ytest), Nt, D, ls, length(ls), sigma_RBF,
                phi_scale, Z, b, n, r, Q, S, scale, meanf, out, curve))
    return meanf, out[], curve
end

# The initial draws of GPTregression for param_seed (GPT_SGLD.jl:357-369): (w, U)
function init_state(n::Integer, r::Integer, D::Integer, Q::Integer, param_seed::Integer;
                    stiefel=true, sigma_w::Real=1.0)
    cfg = Ref(SGLDConfig(n, D, 1, r, Q, 1, 0.0, 0.0, 1.0, sigma_w, 0, 1, UInt64(param_seed),
                         Int32(1), Int32(stiefel), 1, 0))
    w = Array{Float64}(undef, Q); U = Array{Float64}(undef, n, r, D)
    check(ccall((:gpt_sgld_init, LIB), Cint, (Ref{SGLDConfig}, Ptr{Float64}, Ptr{Float64}), cfg, w, U))
    return w, U
end

# GPNT_SGLD(phi,y,signal_var,sigma_theta,m,eps_theta,decay_rate,burnin,maxepoch,param_seed)
# GPT_SGLD.jl:809
function GPNT_SGLD(phi::Array{Float64,2}, y::Array{Float64}, signal_var::Real, sigma_theta::Real,
                   m::Integer, eps_theta::Real, decay_rate::Real, burnin::Integer, maxepoch::Integer,
                   param_seed::Integer)
    n, N = size(phi)
    store = Array{Float64}(undef, n, (maxepoch + burnin) * cld(N, m))
    rc = ccall((:gpt_gpnt_sgld, LIB), Cint,
               (Ptr{Float64}, Ptr{Float64}, Int64, Int64, Float64, Float64, Int64, Float64, Float64,
                Int64, Int64, UInt64, Ptr{Float64}),
               phi, vec(y), n, N, signal_var, sigma_theta, m, eps_theta, decay_rate, burnin, maxepoch,
               param_seed, store)
    if rc == 4
        println("Get NaN in theta. Try smaller epsilon")
        return zeros(n)
    end
    check(rc)
    return store
end

# Sibling GPNT_SGLD chains on one phi / y (step-size, noise and seed sweeps of
# PowerPlantNoTensorExperiment.jl / kin40kNoTensorExperiment.jl): chain k runs GPNT_SGLD with
# signal_vars[k], sigma_thetas[k], eps_thetas[k], seeds[k].  (theta_store (n, kept, nchains),
# status (nchains)); store_every keeps the 1-based steps divisible by it (cld(N, m): the epoch ends)
function GPNT_SGLD_chains(phi::Array{Float64,2}, y::Array{Float64}, signal_vars::Vector{Float64},
                          sigma_thetas::Vector{Float64}, m::Integer, eps_thetas::Vector{Float64},
                          decay_rate::Real, burnin::Integer, maxepoch::Integer,
                          seeds::Vector{UInt64}; store_every::Integer=1)
    n, N = size(phi); nch = length(seeds)
    length(y) == N || error("phi and y disagree on N")
    for (name, v) in (("signal_vars", signal_vars), ("sigma_thetas", sigma_thetas),
                      ("eps_thetas", eps_thetas))
        length(v) == nch || error("$name must have one entry per chain (length(seeds) = $nch)")
    end
    store_every >= 1 || error("store_every must be >= 1")
    kept = div((maxepoch + burnin) * cld(N, m), store_every)
    store = zeros(Float64, n, kept, nch); status = zeros(Int32, nch)
    check(ccall((:gpt_gpnt_sgld_chains, LIB), Cint,
                (Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64},
                 Ptr{Float64}, Float64, Int64, Int64, Ptr{UInt64}, Int32, Int64, Ptr{Float64},
                 Ptr{Int32}),
                phi, vec(y), n, N, m, signal_vars, sigma_thetas, eps_thetas, decay_rate, burnin,
                maxepoch, seeds, nch, store_every, store, status))
    return store, status
end

# The same with phi = featureNotensor(X, length_scale, sigma_RBF, Z, b) formed on the device
function GPNT_SGLD_chains_x(X::Array{Float64,2}, y::Array{Float64}, length_scale, sigma_RBF::Real,
                            Z::Array{Float64,2}, b::Array{Float64}, signal_vars::Vector{Float64},
                            sigma_thetas::Vector{Float64}, m::Integer, eps_thetas::Vector{Float64},
                            decay_rate::Real, burnin::Integer, maxepoch::Integer,
                            seeds::Vector{UInt64}; store_every::Integer=1)
    N, D = size(X); n = size(Z, 1); nch = length(seeds)
    ls = collect(Float64, length_scale isa Real ? [length_scale] : length_scale)
    length(y) == N || error("X and y disagree on N")
    (size(Z, 2) == D && length(b) == n) || error("Z must be (n, D) and b of length n")
    (length(ls) == 1 || length(ls) == D) || error("dimensions of X and length_scale do not match")
    for (name, v) in (("signal_vars", signal_vars), ("sigma_thetas", sigma_thetas),
                      ("eps_thetas", eps_thetas))
        length(v) == nch || error("$name must have one entry per chain (length(seeds) = $nch)")
    end
    store_every >= 1 || error("store_every must be >= 1")
    kept = div((maxepoch + burnin) * cld(N, m), store_every)
    store = zeros(Float64, n, kept, nch); status = zeros(Int32, nch)
    check(ccall((:gpt_gpnt_sgld_chains_x, LIB), Cint,
                (Ptr{Float64}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Float64,
                 Ptr{Float64}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                 Float64, Int64, Int64, Ptr{UInt64}, Int32, Int64, Ptr{Float64}, Ptr{Int32}),
                X, vec(y), N, D, ls, length(ls), sigma_RBF, Z, vec(b), n, m, signal_vars,
                sigma_thetas, eps_thetas, decay_rate, burnin, maxepoch, seeds, nch, store_every,
                store, status))
    return store, status
end

# The evaluation of GPNT_SGLD samples (PowerPlantNoTensorExperiment.jl:51-63): the test RMSE of
# every sample, the prediction averaged over `window` (1-based, inclusive, as 60:100 there) and
# its test RMSE, all times `scale`
struct RegEval
    sample_rmse::Vector{Float64}; mean_fhat::Vector{Float64}; rmse::Float64
    scores::Array{Float64,2}
end

# theta_store (n, T) samples of one chain, phitest (n, Ntest)
function GPNT_pred(theta_store::Array{Float64,2}, phitest::Array{Float64,2}, ytest::Array{Float64};
                   window=nothing, scale::Real=1.0)
    n, T = size(theta_store); Nt = size(phitest, 2); a, b = class_window(window, T)
    size(phitest, 1) == n || error("theta_store and phitest disagree on n")
    length(ytest) == Nt || error("ytest must have one target per test row")
    0 <= a < b <= T || error("the window must lie in 1:$T")
    sr = Array{Float64}(undef, T); mf = Array{Float64}(undef, Nt); rm = Array{Float64}(undef, 1)
    sc = Array{Float64}(undef, Nt, T)
    check(ccall((:gpt_gpnt_pred, LIB), Cint,
                (Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Int64, Int64,
                 Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                theta_store, phitest, vec(ytest), n, Nt, T, a, b, scale, sr, mf, rm, sc))
    return RegEval(sr, mf, rm[1], sc)
end

# The same with phitest = featureNotensor(Xtest, length_scale, sigma_RBF, Z, b) formed on the device
function GPNT_pred_x(theta_store::Array{Float64,2}, Xtest::Array{Float64,2}, ytest::Array{Float64},
                     length_scale, sigma_RBF::Real, Z::Array{Float64,2}, bfeat::Array{Float64};
                     window=nothing, scale::Real=1.0)
    n, T = size(theta_store); Nt, D = size(Xtest); a, b = class_window(window, T)
    ls = collect(Float64, length_scale isa Real ? [length_scale] : length_scale)
    (size(Z) == (n, D) && length(bfeat) == n) || error("Z must be (n, D) and b of length n")
    (length(ls) == 1 || length(ls) == D) || error("dimensions of Xtest and length_scale do not match")
    length(ytest) == Nt || error("ytest must have one target per test row")
    0 <= a < b <= T || error("the window must lie in 1:$T")
    sr = Array{Float64}(undef, T); mf = Array{Float64}(undef, Nt); rm = Array{Float64}(undef, 1)
    sc = Array{Float64}(undef, Nt, T)
    check(ccall((:gpt_gpnt_pred_x, LIB), Cint,
                (Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64,
                 Float64, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Int64, Float64,
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                theta_store, Xtest, vec(ytest), Nt, D, ls, length(ls), sigma_RBF, Z, vec(bfeat), n,
                T, a, b, scale, sr, mf, rm, sc))
    return RegEval(sr, mf, rm[1], sc)
end

# The posterior predictive of stored regression samples over `window` (1-based, inclusive) at noise
# variance signal_var: ymu = fmu and fs2 the mean and variance of the predictions over the window,
# ys2 = fs2 + signal_var, lp the moment-matched and lp_mix the Monte-Carlo log density of ytest
# (arrays in the model's units); mnlp, mnlp_mix = -mean(lp), -mean(lp_mix) + log(scale); coverage95
# the share of rows within 1.96 sqrt(ys2) of ymu; rmse, sample_rmse as GPNT_pred's; sample_loglik
# the Gaussian log likelihood of ytest under every sample (lkhdLearningCurve.jl:53)
struct PredictiveEval
    ymu::Vector{Float64}; ys2::Vector{Float64}; fmu::Vector{Float64}; fs2::Vector{Float64}
    lp::Vector{Float64}; lp_mix::Vector{Float64}; mnlp::Float64; mnlp_mix::Float64
    coverage95::Float64; rmse::Float64; sample_rmse::Vector{Float64}; sample_loglik::Vector{Float64}
end

struct PredictiveOut
    fmu::Vector{Float64}; fs2::Vector{Float64}; lp::Vector{Float64}; lpmix::Vector{Float64}
    sums::Vector{Float64}; covered::Vector{Float64}; rmse::Vector{Float64}; srm::Vector{Float64}
end
PredictiveOut(Nt, T) = PredictiveOut(zeros(Nt), zeros(Nt), zeros(Nt), zeros(Nt), zeros(2), zeros(1),
                                     zeros(1), zeros(T))

function predictive_result(o::PredictiveOut, Nt, signal_var, scale)
    sse = Nt .* (o.srm ./ scale) .^ 2
    return PredictiveEval(o.fmu, o.fs2 .+ signal_var, o.fmu, o.fs2, o.lp, o.lpmix,
                          -o.sums[1] / Nt + log(scale), -o.sums[2] / Nt + log(scale),
                          o.covered[1] / Nt, o.rmse[1], o.srm,
                          -sse ./ (2 * signal_var) .- Nt / 2 * log(2 * pi * signal_var))
end

# scores (Ntest, T): one column of predictions per sample
function predictive(scores::Array{Float64,2}, ytest::Array{Float64}, signal_var::Real;
                    window=nothing, scale::Real=1.0)
    Nt, T = size(scores); a, b = class_window(window, T)
    length(ytest) == Nt || error("ytest must have one target per test row")
    0 <= a < b <= T || error("the window must lie in 1:$T")
    o = PredictiveOut(Nt, T)
    check(ccall((:gpt_predictive, LIB), Cint,
                (Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Int64, Float64, Ptr{Float64},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                 Ptr{Float64}),
                scores, vec(ytest), Nt, T, a, b, signal_var, o.fmu, o.fs2, o.lp, o.lpmix, o.sums,
                o.covered, o.rmse, o.srm))
    o.rmse .*= scale; o.srm .*= scale
    return predictive_result(o, Nt, signal_var, scale)
end

# ---- chain diagnostics of a store: split R-hat, ESS, autocorrelation (gpt_chain_diag) ----
struct ChainDiag
    mean::Vector{Float64}; sd::Vector{Float64}; rhat::Vector{Float64}; ess::Vector{Float64}
    mcse::Vector{Float64}; tau::Vector{Float64}; truncated::Vector{Int32}
    chain_mean::Array{Float64,2}; chain_var::Array{Float64,2}
    acf::Union{Nothing,Array{Float64,2}}; chain_acf::Union{Nothing,Array{Float64,3}}
    max_rhat::Float64; min_ess::Float64; n_truncated::Int
end

# store (P, T, M): parameter or test row, kept sample, chain ((P, T): one chain).  window = a:b
# selects the samples (1-based, default all; at least 4), max_lag defaults to min(S - 1, 256).
# truncated[p] == 1: the lags ran out before Geyer's sequence turned negative; ess[p] is then an
# upper bound.  A constant parameter has NaN rhat, ess, mcse, tau and acf.
function chain_diagnostics(store::Array{Float64}; window=nothing, max_lag=nothing, acf::Bool=false,
                           chain_acf::Bool=false)
    ndims(store) in (2, 3) || error("store must be (P, T) or (P, T, M)")
    P, T = size(store, 1), size(store, 2); M = size(store, 3); a, b = class_window(window, T)
    length(store) == P * T * M || error("store must hold P*T*M values")
    0 <= a < b <= T || error("the window must lie in 1:$T")
    b - a >= 4 || error("the window needs at least 4 samples")
    S = b - a; lag = max_lag === nothing ? min(S - 1, 256) : Int(max_lag); K = min(lag, S - 1)
    1 <= lag <= 4096 || error("max_lag must be in 1:4096")
    rows = [zeros(P) for _ = 1:6]; tr = zeros(Int32, P); cm = zeros(P, M); cv = zeros(P, M)
    ac = acf ? zeros(P, K + 1) : nothing; ca = chain_acf ? zeros(P, K + 1, M) : nothing
    check(ccall((:gpt_chain_diag, LIB), Cint,
                (Ptr{Float64}, Int64, Int64, Int64, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                store, P, T, M, a, b, lag, rows[1], rows[2], rows[3], rows[4], rows[5], rows[6], tr,
                cm, cv, ac === nothing ? C_NULL : ac, ca === nothing ? C_NULL : ca))
    live = .!isnan.(rows[3])
    return ChainDiag(rows[1], rows[2], rows[3], rows[4], rows[5], rows[6], tr, cm, cv, ac, ca,
                     any(live) ? maximum(rows[3][live]) : NaN, any(live) ? minimum(rows[4][live]) : NaN,
                     Int(sum(tr)))
end

# GPTregression's stored samples w_store (Q, S), U_store (n, r, D, S) on phitest (n, D, Ntest)
function pred_predictive(w_store::Array{Float64,2}, U_store::Array{Float64,4}, I::Array{Int32,2},
                         phitest::Array{Float64,3}, ytest::Array{Float64}, signal_var::Real;
                         window=nothing, scale::Real=1.0)
    n, D, Nt = size(phitest); r = size(U_store, 2); Q, S = size(w_store); a, b = class_window(window, S)
    size(U_store) == (n, r, D, S) || error("U_store must be (n, r, D, S)")
    size(I) == (Q, D) || error("I must be (Q, D)")
    length(ytest) == Nt || error("ytest must have one target per test row")
    0 <= a < b <= S || error("the window must lie in 1:$S")
    o = PredictiveOut(Nt, S)
    check(ccall((:gpt_pred_predictive, LIB), Cint,
                (Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Int64, Int64,
                 Int64, Int64, Int64, Int64, Float64, Int64, Int64, Float64, Ptr{Float64},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                 Ptr{Float64}),
                w_store, U_store, I, phitest, vec(ytest), n, D, Nt, r, Q, S, scale, a, b, signal_var,
                o.fmu, o.fs2, o.lp, o.lpmix, o.sums, o.covered, o.rmse, o.srm))
    return predictive_result(o, Nt, signal_var, scale)
end

# The same with the test features formed on the device from Xtest, as pred_mean_x
function pred_predictive_x(w_store::Array{Float64,2}, U_store::Array{Float64,4}, I::Array{Int32,2},
                           Xtest::Array{Float64,2}, ytest::Array{Float64}, length_scale,
                           sigma_RBF::Real, phi_scale::Real, Z::Array{Float64,2}, bfeat::Array{Float64},
                           signal_var::Real; window=nothing, scale::Real=1.0)
    Nt, D = size(Xtest); n = size(Z, 1); r = size(U_store, 2); Q, S = size(w_store)
    a, b = class_window(window, S)
    ls = collect(Float64, length_scale isa Real ? [length_scale] : length_scale)
    size(U_store) == (n, r, D, S) || error("U_store must be (n, r, D, S)")
    size(I) == (Q, D) || error("I must be (Q, D)")
    (size(Z, 2) == D && length(bfeat) == n * D) || error("Z and b must be (n, D)")
    (length(ls) == 1 || length(ls) == D) || error("dimensions of Xtest and length_scale do not match")
    length(ytest) == Nt || error("ytest must have one target per test row")
    0 <= a < b <= S || error("the window must lie in 1:$S")
    o = PredictiveOut(Nt, S)
    check(ccall((:gpt_pred_predictive_x, LIB), Cint,
                (Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Int64, Int64,
                 Ptr{Float64}, Int64, Float64, Float64, Ptr{Float64}, Ptr{Float64}, Int64, Int64,
                 Int64, Int64, Float64, Int64, Int64, Float64, Ptr{Float64}, Ptr{Float64},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                w_store, U_store, I, Xtest, vec(ytest), Nt, D, ls, length(ls), sigma_RBF, phi_scale,
                Z, vec(bfeat), n, r, Q, S, scale, a, b, signal_var, o.fmu, o.fs2, o.lp, o.lpmix,
                o.sums, o.covered, o.rmse, o.srm))
    return predictive_result(o, Nt, signal_var, scale)
end

# GPNT_SGLD's stored samples theta_store (n, T) on phitest (n, Ntest), beside GPNT_pred
function GPNT_predictive(theta_store::Array{Float64,2}, phitest::Array{Float64,2},
                         ytest::Array{Float64}, signal_var::Real; window=nothing, scale::Real=1.0)
    n, T = size(theta_store); Nt = size(phitest, 2); a, b = class_window(window, T)
    size(phitest, 1) == n || error("theta_store and phitest disagree on n")
    length(ytest) == Nt || error("ytest must have one target per test row")
    0 <= a < b <= T || error("the window must lie in 1:$T")
    o = PredictiveOut(Nt, T)
    check(ccall((:gpt_gpnt_predictive, LIB), Cint,
                (Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Int64, Int64,
                 Float64, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                theta_store, phitest, vec(ytest), n, Nt, T, a, b, scale, signal_var, o.fmu, o.fs2,
                o.lp, o.lpmix, o.sums, o.covered, o.rmse, o.srm))
    return predictive_result(o, Nt, signal_var, scale)
end

# The same with phitest = featureNotensor(Xtest, length_scale, sigma_RBF, Z, b) formed on the device
function GPNT_predictive_x(theta_store::Array{Float64,2}, Xtest::Array{Float64,2},
                           ytest::Array{Float64}, length_scale, sigma_RBF::Real, Z::Array{Float64,2},
                           bfeat::Array{Float64}, signal_var::Real; window=nothing, scale::Real=1.0)
    n, T = size(theta_store); Nt, D = size(Xtest); a, b = class_window(window, T)
    ls = collect(Float64, length_scale isa Real ? [length_scale] : length_scale)
    (size(Z) == (n, D) && length(bfeat) == n) || error("Z must be (n, D) and b of length n")
    (length(ls) == 1 || length(ls) == D) || error("dimensions of Xtest and length_scale do not match")
    length(ytest) == Nt || error("ytest must have one target per test row")
    0 <= a < b <= T || error("the window must lie in 1:$T")
    o = PredictiveOut(Nt, T)
    check(ccall((:gpt_gpnt_predictive_x, LIB), Cint,
                (Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64,
                 Float64, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Int64, Float64, Float64,
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                 Ptr{Float64}, Ptr{Float64}),
                theta_store, Xtest, vec(ytest), Nt, D, ls, length(ls), sigma_RBF, Z, vec(bfeat), n,
                T, a, b, scale, signal_var, o.fmu, o.fs2, o.lp, o.lpmix, o.sums, o.covered, o.rmse,
                o.srm))
    return predictive_result(o, Nt, signal_var, scale)
end

# GPNT_SGLDclass(phi,y,sigma_theta,m,eps_theta,decay_rate,burnin,maxepoch,param_seed)
# GPT_SGLD.jl:851 -> theta_store (n, C, (maxepoch+burnin)*numbatches); y holds labels in 1..C
function GPNT_SGLDclass(phi::Array{Float64,2}, y::Array, sigma_theta::Real, m::Integer,
                        eps_theta::Real, decay_rate::Real, burnin::Integer, maxepoch::Integer,
                        param_seed::Integer)
    n, N = size(phi)
    yf = collect(Float64, vec(y))
    ncls = Int(maximum(yf) - minimum(yf) + 1)
    store = Array{Float64}(undef, n, ncls, (maxepoch + burnin) * cld(N, m))
    rc = ccall((:gpt_gpnt_sgld_class, LIB), Cint,
               (Ptr{Float64}, Ptr{Float64}, Int64, Int64, Float64, Int64, Float64, Float64, Int64,
                Int64, UInt64, Ptr{Float64}),
               phi, yf, n, N, sigma_theta, m, eps_theta, decay_rate, burnin, maxepoch, param_seed,
               store)
    if rc == 4
        println("Get NaN in theta. Try smaller epsilon")
        return zeros(n)
    end
    check(rc)
    return store
end

# Sibling GPNT_SGLDclass chains on one phi / y (step-size and seed sweeps,
# ImageNoTensorExperiment.jl:36-38): (theta_store (n, C, kept, nchains), status (nchains));
# store_every keeps the 1-based steps divisible by it (cld(N, m): the epoch ends)
function GPNT_SGLDclass_chains(phi::Array{Float64,2}, y::Array, sigma_theta::Real, m::Integer,
                               eps_thetas::Vector{Float64}, decay_rate::Real, burnin::Integer,
                               maxepoch::Integer, seeds::Vector{UInt64}; store_every::Integer=1)
    n, N = size(phi); nch = length(seeds)
    yf = collect(Float64, vec(y))
    ncls = Int(maximum(yf) - minimum(yf) + 1)
    kept = div((maxepoch + burnin) * cld(N, m), store_every)
    store = zeros(Float64, n, ncls, kept, nch); status = zeros(Int32, nch)
    check(ccall((:gpt_gpnt_sgld_class_chains, LIB), Cint,
                (Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Float64, Int64, Ptr{Float64},
                 Float64, Int64, Int64, Ptr{UInt64}, Int32, Int64, Ptr{Float64}, Ptr{Int32}),
                phi, yf, n, N, ncls, sigma_theta, m, eps_thetas, decay_rate, burnin, maxepoch,
                seeds, nch, store_every, store, status))
    return store, status
end

# The result of the evaluation functions (ImageExperiment.jl:50-72): per-sample prop_missed and
# mean_nlp, the same on the scores averaged over `window` (1-based, inclusive, as 60:100 there),
# those averaged scores, and the prediction and nlp of every test row on them
struct ClassEval
    prop_missed::Vector{Float64}; mean_nlp::Vector{Float64}
    avg_prop_missed::Float64; avg_mean_nlp::Float64
    mean_fhat::Array{Float64,2}; prediction::Vector{Int32}; nlp::Vector{Float64}
    scores::Array{Float64,3}
end
class_window(window, T) = window === nothing ? (0, T) : (first(window) - 1, last(window))

function class_eval(scores::Array{Float64,3}, ytest::Array; window=nothing)
    Nt, ncls, T = size(scores); a, b = class_window(window, T)
    yi = collect(Int32, vec(ytest))
    pm = Array{Float64}(undef, T); nl = Array{Float64}(undef, T); avg = Array{Float64}(undef, 2)
    mf = Array{Float64}(undef, Nt, ncls); pr = Array{Int32}(undef, Nt); np = Array{Float64}(undef, Nt)
    check(ccall((:gpt_class_eval, LIB), Cint,
                (Ptr{Float64}, Ptr{Int32}, Int64, Int64, Int64, Int64, Int64, Ptr{Float64},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}),
                scores, yi, Nt, ncls, T, a, b, pm, nl, avg, mf, pr, np))
    return ClassEval(pm, nl, avg[1], avg[2], mf, pr, np, scores)
end

# theta_store (n, C, T) full-theta samples, phitest (n, Ntest): ImageNoTensorExperiment.jl:50-75
function GPNT_pred_class(theta_store::Array{Float64,3}, phitest::Array{Float64,2}, ytest::Array;
                         window=nothing)
    n, ncls, T = size(theta_store); Nt = size(phitest, 2); a, b = class_window(window, T)
    yi = collect(Int32, vec(ytest))
    pm = Array{Float64}(undef, T); nl = Array{Float64}(undef, T); avg = Array{Float64}(undef, 2)
    mf = Array{Float64}(undef, Nt, ncls); pr = Array{Int32}(undef, Nt); np = Array{Float64}(undef, Nt)
    sc = Array{Float64}(undef, Nt, ncls, T)
    check(ccall((:gpt_gpnt_pred_class, LIB), Cint,
                (Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Int64, Int64, Int64, Int64, Int64, Int64,
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64},
                 Ptr{Float64}),
                theta_store, phitest, yi, n, Nt, ncls, T, a, b, pm, nl, avg, mf, pr, np, sc))
    return ClassEval(pm, nl, avg[1], avg[2], mf, pr, np, sc)
end

# GPTclassification's stores w (Q, C, T), U (n, r, D, C, T), phitest (n, D, Ntest):
# ImageExperiment.jl:50-72 with one upload of phitest
function pred_class(w_store::Array{Float64,3}, U_store::Array{Float64,5}, I::Array{Int32,2},
                    phitest::Array{Float64,3}, ytest::Array; window=nothing)
    n, D, Nt = size(phitest); Q, ncls, T = size(w_store); r = size(U_store, 2)
    a, b = class_window(window, T)
    yi = collect(Int32, vec(ytest))
    pm = Array{Float64}(undef, T); nl = Array{Float64}(undef, T); avg = Array{Float64}(undef, 2)
    mf = Array{Float64}(undef, Nt, ncls); pr = Array{Int32}(undef, Nt); np = Array{Float64}(undef, Nt)
    sc = Array{Float64}(undef, Nt, ncls, T)
    check(ccall((:gpt_pred_class, LIB), Cint,
                (Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}, Int64, Int64,
                 Int64, Int64, Int64, Int64, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}),
                w_store, U_store, I, phitest, yi, n, D, Nt, r, Q, ncls, T, a, b, pm, nl, avg, mf,
                pr, np, sc))
    return ClassEval(pm, nl, avg[1], avg[2], mf, pr, np, sc)
end

# GPNT_nlogmarginal / GPNT_gradnlogmarginal (GPT_SGLD.jl:921-962) with featureNotensor /
# gradfeatureNotensor as the feature closures: X, Z, b take the closures' place.
# hyperparams = [length_scale (D entries, or one); sigma_RBF; signal_var].  A failed Cholesky
# (the reference's PosDefException) is error code 5.
function gpnt_marginal(X::Array{Float64,2}, y::Array{Float64}, Z::Array{Float64,2},
                       b::Array{Float64}, hyperparams::Vector{Float64}, want_grad::Bool)
    N, D = size(X); n = size(Z, 1)
    nlml = Array{Float64}(undef, 1)
    grad = Array{Float64}(undef, length(hyperparams))
    check(ccall((:gpt_gpnt_nlogmarginal, LIB), Cint,
                (Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64,
                 Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}),
                X, N, D, vec(y), Z, vec(b), n, hyperparams, length(hyperparams), Int64(want_grad),
                nlml, grad))
    return nlml[1], grad
end
GPNT_nlogmarginal(X, y, Z, b, hyperparams) = gpnt_marginal(X, y, Z, b, hyperparams, false)[1]
GPNT_gradnlogmarginal(X, y, Z, b, hyperparams) = gpnt_marginal(X, y, Z, b, hyperparams, true)[2]

# The closed-form predictive of the same model at hyperparams: (ymu, ys2, fmu, fs2, lp) as
# GP_predict returns it, with fmu = phi*'l and fs2 = signal_var * colsum((L^-1 phi*).^2);
# lp is nothing without ytest
function GPNT_predict(X::Array{Float64,2}, y::Array{Float64}, Z::Array{Float64,2},
                      b::Array{Float64}, hyperparams::Vector{Float64}, Xtest::Array{Float64,2},
                      ytest=nothing)
    N, D = size(X); n = size(Z, 1); Ntest = size(Xtest, 1)
    size(Z, 2) == D || error("Z must be (n, D)")
    length(b) == n || error("b must have n entries")
    length(y) == N || error("y must have N entries")
    size(Xtest, 2) == D || error("Xtest must be (Ntest, D)")
    fmu = Array{Float64}(undef, Ntest); fs2 = Array{Float64}(undef, Ntest)
    yt = ytest === nothing ? Float64[] : Vector{Float64}(vec(ytest))
    (ytest === nothing || length(yt) == Ntest) || error("ytest must have Ntest entries")
    lpv = Array{Float64}(undef, ytest === nothing ? 0 : Ntest)
    GC.@preserve yt lpv begin
        yp = ytest === nothing ? Ptr{Float64}(C_NULL) : pointer(yt)
        lpp = ytest === nothing ? Ptr{Float64}(C_NULL) : pointer(lpv)
        check(ccall((:gpt_gpnt_predict, LIB), Cint,
                    (Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64,
                     Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64},
                     Ptr{Float64}, Ptr{Float64}),
                    X, N, D, vec(y), Z, vec(b), n, hyperparams, length(hyperparams), Xtest, Ntest,
                    yp, fmu, fs2, lpp))
    end
    lp = ytest === nothing ? nothing : lpv
    return fmu, fs2 .+ hyperparams[end], fmu, fs2, lp
end

# PowerPlantDataExperiment.jl:47-97: (FrobError = |K - phi'phi|_F, |K|_F, max|K - phi'phi|) with K
# the exact squared-exponential kernel matrix of X at hyperparams and phi = featureNotensor(X, ...)
function RFF_kernel_error(X::Array{Float64,2}, Z::Array{Float64,2}, b::Array{Float64},
                          hyperparams::Vector{Float64})
    N, D = size(X); n = size(Z, 1)
    size(Z, 2) == D || error("Z must be (n, D)")
    length(b) == n || error("b must have n entries")
    out = Array{Float64}(undef, 3)
    check(ccall((:gpt_rff_kernel_error, LIB), Cint,
                (Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64},
                 Int64, Ptr{Float64}),
                X, N, D, Z, vec(b), n, hyperparams, length(hyperparams), out))
    return out[1], out[2], out[3]
end

# Exact GP regression (GP_nlogmarginal GPT_SGLD.jl:905-915; GPkit InfExact / prediction with
# CovSEiso or CovSEard, LikGauss, zero mean).  hyperparams = [length_scale (D entries, or one);
# sigma_RBF; signal_var]; GPkit's dnlZ is GP_gradnlogmarginal .* [l...; sigma_RBF; 2 signal_var].
function gp_marginal(X::Array{Float64,2}, y::Array{Float64}, hyperparams::Vector{Float64},
                     want_grad::Bool)
    N, D = size(X)
    nlml = Array{Float64}(undef, 1)
    grad = Array{Float64}(undef, length(hyperparams))
    check(ccall((:gpt_gp_nlogmarginal, LIB), Cint,
                (Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Int64,
                 Ptr{Float64}, Ptr{Float64}),
                X, N, D, vec(y), hyperparams, length(hyperparams), Int64(want_grad), nlml, grad))
    return nlml[1], grad
end
# the reference's signature: sigma_RBF2 is sigma_RBF squared, length_scale a scalar or D entries
GP_nlogmarginal(X, y, signal_var, sigma_RBF2, length_scale) =
    gp_marginal(X, y, Float64[length_scale...; sqrt(sigma_RBF2); signal_var], false)[1]
GP_gradnlogmarginal(X, y, hyperparams) = gp_marginal(X, y, hyperparams, true)[2]

# GPkit's prediction: (ymu, ys2, fmu, fs2, lp); lp is nothing without ytest
function GP_predict(X::Array{Float64,2}, y::Array{Float64}, hyperparams::Vector{Float64},
                    Xtest::Array{Float64,2}, ytest=nothing)
    N, D = size(X); Ntest = size(Xtest, 1)
    size(Xtest, 2) == D || error("Xtest must be (Ntest, D)")
    fmu = Array{Float64}(undef, Ntest); fs2 = Array{Float64}(undef, Ntest)
    yt = ytest === nothing ? Float64[] : Vector{Float64}(vec(ytest))
    lpv = Array{Float64}(undef, ytest === nothing ? 0 : Ntest)
    GC.@preserve yt lpv begin
        yp = ytest === nothing ? Ptr{Float64}(C_NULL) : pointer(yt)
        lpp = ytest === nothing ? Ptr{Float64}(C_NULL) : pointer(lpv)
        check(ccall((:gpt_gp_predict, LIB), Cint,
                    (Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64},
                     Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                    X, N, D, vec(y), hyperparams, length(hyperparams), Xtest, Ntest, yp, fmu, fs2,
                    lpp))
    end
    lp = ytest === nothing ? nothing : lpv
    return fmu, fs2 .+ hyperparams[end], fmu, fs2, lp
end

# Function draws (GaussianProcess.jl:66-122).  GPrand: S draws R'z, R = chol(K + jitter*I), of the
# zero-mean squared-exponential GP at X (N, D), from Philox stream 25; length_scale is a scalar or D
# entries.  Returns (N, S).
function GPrand(X::Array{Float64,2}, length_scale, sigma_RBF::Real; S::Integer=1, seed::Integer=0,
                jitter::Real=1e-6)
    N, D = size(X)
    hyperparams = Float64[length_scale...; sigma_RBF; 1.0]
    F = Array{Float64}(undef, N, S)
    check(ccall((:gpt_gp_rand, LIB), Cint,
                (Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Float64, Int64, UInt64,
                 Ptr{Float64}),
                X, N, D, hyperparams, length(hyperparams), jitter, S, UInt64(seed), F))
    return F
end

# GPpost followed by GPrand: (fmu, samples (Ntest, S), cov (Ntest, Ntest)) of the posterior GP at
# Xtest; samples = fmu + L z, L L' = cov + jitter*I (observed: + signal_var*I); z (Ntest, S)
# replaces the Philox normals
function GPpost_rand(X::Array{Float64,2}, y::Array{Float64}, hyperparams::Vector{Float64},
                     Xtest::Array{Float64,2}; S::Integer=1, seed::Integer=0, jitter::Real=1e-6,
                     observed::Bool=false, z=nothing)
    N, D = size(X); Ntest = size(Xtest, 1)
    size(Xtest, 2) == D || error("Xtest must be (Ntest, D)")
    length(y) == N || error("y must have N entries")
    fmu = Array{Float64}(undef, Ntest); F = Array{Float64}(undef, Ntest, S)
    cov = Array{Float64}(undef, Ntest, Ntest)
    zin = z === nothing ? Float64[] : Array{Float64}(z)
    z === nothing || size(zin) == (Ntest, S) || error("z must be (Ntest, S)")
    GC.@preserve zin begin
        zp = z === nothing ? Ptr{Float64}(C_NULL) : pointer(zin)
        check(ccall((:gpt_gp_post_rand, LIB), Cint,
                    (Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64},
                     Int64, Float64, Int32, Int64, UInt64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                     Ptr{Float64}),
                    X, N, D, vec(y), hyperparams, length(hyperparams), Xtest, Ntest, jitter,
                    Int32(observed), S, UInt64(seed), zp, fmu, F, cov))
    end
    return fmu, F, cov
end

# S exact draws (n, S) from the posterior theta | y ~ N(l, signal_var*A^-1) of GPNT_nlogmarginal's
# model: a GPNT_SGLD store for GPNT_pred / GPNT_predictive
function GPNT_draw_theta(X::Array{Float64,2}, y::Array{Float64}, Z::Array{Float64,2},
                         b::Array{Float64}, hyperparams::Vector{Float64}, S::Integer;
                         seed::Integer=0, z=nothing)
    N, D = size(X); n = size(Z, 1)
    size(Z, 2) == D || error("Z must be (n, D)")
    length(b) == n || error("b must have n entries")
    length(y) == N || error("y must have N entries")
    theta = Array{Float64}(undef, n, S)
    zin = z === nothing ? Float64[] : Array{Float64}(z)
    z === nothing || size(zin) == (n, S) || error("z must be (n, S)")
    GC.@preserve zin begin
        zp = z === nothing ? Ptr{Float64}(C_NULL) : pointer(zin)
        check(ccall((:gpt_gpnt_draw_theta, LIB), Cint,
                    (Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64,
                     Ptr{Float64}, Int64, Int64, UInt64, Ptr{Float64}, Ptr{Float64}),
                    X, N, D, vec(y), Z, vec(b), n, hyperparams, length(hyperparams), S,
                    UInt64(seed), zp, theta))
    end
    return theta
end

# createmesh(interval_start,interval_end,npts)  GPT_SGLD.jl:289-301
function createmesh(interval_start, interval_end, npts)
    x = collect(range(interval_start, stop=interval_end, length=npts))
    y = collect(range(interval_start, stop=interval_end, length=npts))
    grid = Array{Float64}(undef, npts^2, 2); k = 1
    for i = 1:npts, j = 1:npts
        grid[k, 1] = x[i]; grid[k, 2] = y[j]; k += 1
    end
    return x, y, grid
end

# fhatdraw(X,n,length_scale,sigma_RBF,r,Q)  GPT_SGLD.jl:304-342, seeded: (y, w, U, I, phi)
function fhatdraw(X::Array{Float64,2}, n::Integer, length_scale, sigma_RBF::Real, r::Integer,
                  Q::Integer; seed::Integer=0)
    N, D = size(X)
    (length_scale isa Real || length(length_scale) == D) ||
        error("dimensions of X and length_scale do not match")
    phi = feature(X, n, length_scale, sigma_RBF, seed, sqrt(n / Q^(1 / D)))
    w, U = init_state(n, r, D, Q, seed; stiefel=true, sigma_w=1.0)
    I = samplenz(r, D, Q, seed)
    return pred(w, U, I, phi), w, U, I, phi
end

# The joint likelihood of the full-theta softmax classifier (neglogjointlkhd /
# gradneglogjointlkhd, ImageExperiment.jl:135-204; the objective of GPNT_hyperparameters_ng,
# GPT_SGLD.jl:1005-1063): X, y, Z, b take the closures' place.  theta_vec has n*C entries
# (vec of the n x C matrix), hyperparams = [length_scale (D entries, or one); sigma_RBF], labels are
# integers in 1..C (C defaults to max - min + 1 and may be passed when a class is absent).  Every
# length is checked here, before the library reads the arrays.
function joint_dims(X::Array{Float64,2}, y::Array, Z::Array{Float64,2}, b::Array{Float64},
                    theta_vec::Array{Float64}, hyperparams::Vector{Float64}, C::Integer)
    N, D = size(X); n = size(Z, 1)
    size(Z, 2) == D || error("Z must be (n, D)")
    length(b) == n || error("b must have n entries")
    length(y) == N || error("y must have N entries")
    length(theta_vec) == n * C || error("theta_vec must have n*C entries")
    (length(hyperparams) == 2 || length(hyperparams) == D + 1) ||
        error("hyperparams must have 2 or D + 1 entries")
    return N, D, n
end
joint_classes(y, C) = C === nothing ? Int(maximum(y) - minimum(y) + 1) : Int(C)

function gpnt_joint(X::Array{Float64,2}, y::Array, Z::Array{Float64,2}, b::Array{Float64},
                    theta_vec::Array{Float64}, hyperparams::Vector{Float64}, want_grad::Bool;
                    C=nothing)
    ncls = joint_classes(y, C)
    N, D, n = joint_dims(X, y, Z, b, theta_vec, hyperparams, ncls)
    yf = collect(Float64, vec(y))
    value = Array{Float64}(undef, 1)
    grad = Array{Float64}(undef, n * ncls + length(hyperparams))
    check(ccall((:gpt_gpnt_neglogjoint, LIB), Cint,
                (Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Int64,
                 Ptr{Float64}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}),
                X, N, D, yf, ncls, Z, vec(b), n, vec(theta_vec), hyperparams, length(hyperparams),
                Int64(want_grad), value, grad))
    return value[1], grad
end
# the reference's closures: neglogjointlkhd(theta_vec, hyperparams), gradneglogjointlkhd(...) ->
# [vec(gradtheta); gradlength_scale; gradsigma_RBF]
neglogjointlkhd(X, y, Z, b, theta_vec, hyperparams; C=nothing) =
    gpnt_joint(X, y, Z, b, theta_vec, hyperparams, false; C=C)[1]
gradneglogjointlkhd(X, y, Z, b, theta_vec, hyperparams; C=nothing) =
    gpnt_joint(X, y, Z, b, theta_vec, hyperparams, true; C=C)[2]

# nsteps Langevin steps on theta at hyperparams from the 0-based step t0 (the E step of
# GPNT_hyperparameters_ng, GPT_SGLD.jl:1031-1033); returns the new theta_vec.  Error code 4: theta
# turned non-finite.
function joint_langevin(X::Array{Float64,2}, y::Array, Z::Array{Float64,2}, b::Array{Float64},
                        theta_vec::Array{Float64}, hyperparams::Vector{Float64}, epsilon::Real,
                        nsteps::Integer, seed::Integer; t0::Integer=0, C=nothing)
    ncls = joint_classes(y, C)
    N, D, n = joint_dims(X, y, Z, b, theta_vec, hyperparams, ncls)
    (nsteps >= 0 && t0 >= 0) || error("nsteps and t0 must not be negative")
    yf = collect(Float64, vec(y))
    theta = collect(Float64, vec(theta_vec))
    check(ccall((:gpt_gpnt_joint_langevin, LIB), Cint,
                (Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Int64,
                 Ptr{Float64}, Ptr{Float64}, Int64, Float64, Int64, UInt64, Int64),
                X, N, D, yf, ncls, Z, vec(b), n, theta, hyperparams, length(hyperparams),
                epsilon, nsteps, UInt64(seed), t0))
    return theta
end

# burnin + nsamples Hamiltonian Monte Carlo transitions on theta at hyperparams from the 0-based
# transition t0: L leapfrog steps of size sqrt(epsilon) and a Metropolis test (L = 1: the MALA loop
# of BloodTransfusionExperiment.jl:255-278).  Returns (theta_vec after the run, theta_store
# (n, C, nsamples ÷ thin), accept, dH, value, ndivergent); accept, dH = H0 - H1 and value = U of
# the kept state have one entry per transition.  Error code 4: the starting theta is not finite.
function joint_hmc(X::Array{Float64,2}, y::Array, Z::Array{Float64,2}, b::Array{Float64},
                   theta_vec::Array{Float64}, hyperparams::Vector{Float64}, epsilon::Real,
                   L::Integer, nsamples::Integer, seed::Integer; burnin::Integer=0,
                   thin::Integer=1, t0::Integer=0, C=nothing)
    ncls = joint_classes(y, C)
    N, D, n = joint_dims(X, y, Z, b, theta_vec, hyperparams, ncls)
    (nsamples >= 0 && burnin >= 0 && t0 >= 0) || error("nsamples, burnin and t0 must not be negative")
    (thin >= 1 && L >= 1) || error("thin and L must be at least 1")
    yf = collect(Float64, vec(y))
    theta = collect(Float64, vec(theta_vec))
    ntrans = burnin + nsamples
    store = Array{Float64}(undef, n, ncls, div(nsamples, thin))
    accept = Array{Int32}(undef, ntrans)
    dH = Array{Float64}(undef, ntrans)
    value = Array{Float64}(undef, ntrans)
    ndiv = Array{Int32}(undef, 1)
    check(ccall((:gpt_gpnt_joint_hmc, LIB), Cint,
                (Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Int64,
                 Ptr{Float64}, Ptr{Float64}, Int64, Float64, Int64, Int64, Int64, Int64, UInt64,
                 Int64, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                X, N, D, yf, ncls, Z, vec(b), n, theta, hyperparams, length(hyperparams),
                epsilon, L, burnin, nsamples, thin, UInt64(seed), t0, store, accept, dH, value,
                ndiv))
    return theta, store, accept, dH, value, Int(ndiv[1])
end
joint_mala(X, y, Z, b, theta_vec, hyperparams, epsilon, nsamples, seed; kw...) =
    joint_hmc(X, y, Z, b, theta_vec, hyperparams, epsilon, 1, nsamples, seed; kw...)

# scores (Ntest, C) = featureNotensor(Xtest)' * theta at hyperparams: class_eval's input
# (reshape to (Ntest, C, 1)), the prop_missed / mean_nlp line of ImageExperiment.jl:258-268
function joint_scores(Xtest::Array{Float64,2}, Z::Array{Float64,2}, b::Array{Float64},
                      theta::Array{Float64,2}, hyperparams::Vector{Float64})
    Nt, D = size(Xtest); n, ncls = size(theta)
    size(Z) == (n, D) || error("Z must be (n, D)")
    length(b) == n || error("b must have n entries")
    (length(hyperparams) == 2 || length(hyperparams) == D + 1) ||
        error("hyperparams must have 2 or D + 1 entries")
    scores = Array{Float64}(undef, Nt, ncls)
    check(ccall((:gpt_gpnt_joint_scores, LIB), Cint,
                (Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64},
                 Ptr{Float64}, Int64, Ptr{Float64}),
                Xtest, Nt, D, ncls, Z, vec(b), n, theta, hyperparams, length(hyperparams), scores))
    return scores
end

end # module
