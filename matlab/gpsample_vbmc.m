function X = gpsample_vbmc(vp,gp,Ns,origflag)
%GPSAMPLE_VBMC Drop-in shim: samples of the GP surrogate on an MI355X ('gp_surrogate_sample': vbmc_gp_surrogate_sample).
%
% Same signature and defaulting as the reference (misc/gpsample_vbmc.m).  It is reached by the reference's own vbmc_rnd(vp,N,origflag,'gp')
% -- to which vbmc_hip_rnd falls through for 'gp' -- by path lookup.  One call runs the noise estimate over the variational posterior
% (where the GP carries s2), the 2(D+1) starting walkers drawn from vp, the 'parallel' chain of gplite_sample on its default box
% and the way back to the original space.  Here: the O(N D S) set-up the library leaves to its caller -- the geometric-mean length
% scale, the rescaled inputs, the training noise averaged over hyper-samples -- and the box.  The random numbers are the library's,
% keyed by one randi of MATLAB's stream.  The sampler is the library's ensemble slice sampler, not eissample_lite's own moves.
%
% Falls through to the reference function on a 'vbmc_hip:unsupported' answer of the library (a GP beyond the range in which the
% prediction keeps inv(L') resident, other transform types, covariance or mean functions, D beyond the limits).
if nargin < 4 || isempty(origflag); origflag = true; end
try
    [N,D] = size(gp.X);
    S = numel(gp.post);
    noise = [];
    if isfield(gp,'s2') && ~isempty(gp.s2)
        hyp = [gp.post.hyp];
        noise.gplengthscale = exp(sum(hyp(1:D,:),2)'/S);
        noise.X_rescaled = bsxfun(@rdivide,gp.X,noise.gplengthscale);
        tot = zeros(N,1);
        for s = 1:S
            tot = tot + gplite_noisefun(hyp(gp.Ncov+(1:gp.Nnoise),s),gp.X,gp.noisefun,gp.y,gp.s2);
        end
        noise.sn2new = tot/S;
    end
    lo = min(gp.X,[],1); hi = max(gp.X,[],1);
    opts.S = S;
    opts.Seed = randi(2^31-1);
    X = vbmc_hip_mex('gp_surrogate_sample',vbmc_hip_gp_handle(gp),vp,Ns,double(origflag),lo-10*(hi-lo),hi+10*(hi-lo),noise,opts);
catch err
    if ~strcmp(err.identifier,'vbmc_hip:unsupported'); rethrow(err); end
    ref = vbmc_hip_reference('gpsample_vbmc');
    X = ref(vp,gp,Ns,origflag);
end
end
