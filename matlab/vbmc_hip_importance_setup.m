function [ais,ok] = vbmc_hip_importance_setup(vp,gp,acqfun,options)
%VBMC_HIP_IMPORTANCE_SETUP Steps 1 and 2 of private/activeimportancesampling_vbmc.m (:106-235) on an MI355X for acqimiqr_vbmc in one
%   call ('is_setup': vbmc_acq_is_setup): the draws from the smoothed variational posterior and from the boxes around the training
%   inputs, their prediction and importance weights, the resampling of the starting walkers, the MCMC per GP hyper-sample, the closing
%   prediction and the device state of the result.
%
%   [ais,ok] = vbmc_hip_importance_setup(vp,gp,acqfun,options)
%
% stands where the else-branch of activeimportancesampling_vbmc.m stands ("Step 1" to the end of the loop over the GP hyper-samples).
% The struct comes back with Xa (Nm x D x S), lnw (S x Nm) and fs2a (Nm x S) filled -- with ActiveImportanceSamplingMCMCSamples = 0
% the Step 1 arrays Xa (Na x D), lnw (S x Na), fs2a (Na x S) -- and its device state registered with vbmc_hip_is_handle, so that the
% acquisition calls of this active-sampling step upload nothing.  The random numbers are the library's, keyed by one randi of MATLAB's
% stream.  vbmc_hip_importance_sample(vp,gp,acqfun,options) is the same call.
%
% A starting walker of zero density (n_bad > 0) hands the Step 1 arrays to vbmc_hip_importance_sample, which resamples on the host.
%
% ok = false (the caller runs its own code): an acquisition function other than acqimiqr_vbmc, importance_sampling_vp, vp.delta > 0,
% an unsupported GP model or mixture, or a 'vbmc_hip:unsupported' answer of the library.
ais = struct('lnw',[],'Xa',[],'fs2a',[]);
ok = false;
info = acqfun('info');
supported = strcmp(func2str(acqfun),'acqimiqr_vbmc') ...
    && ~(isfield(info,'importance_sampling_vp') && info.importance_sampling_vp) ...
    && ~(isfield(vp,'delta') && ~isempty(vp.delta) && any(vp.delta(:) ~= 0)) ...
    && vbmc_hip_supported(gp,vp,true) && gp.noisefun(3) == 0;
if ~supported; return; end
nsamples = max(options.ActiveImportanceSamplingMCMCSamples,0);
opts = struct('Thin',options.ActiveImportanceSamplingMCMCThin,'Burnin',-1,'Spec',0,'Seed',randi(2^31-1),'Chunk',0,'S',numel(gp.post));
h = vbmc_hip_gp_handle(gp);
try
    [Xa,lnw,fs2a,his,out] = vbmc_hip_mex('is_setup',h,vp,options.ActiveImportanceSamplingVPSamples,options.ActiveImportanceSamplingBoxSamples,nsamples,opts);
catch err
    if ~strcmp(err.identifier,'vbmc_hip:unsupported'); rethrow(err); end
    return;
end
if nsamples == 0
    ais.Xa = out.Xa1;
    ais.lnw = out.lnw1;
    ais.fs2a = out.fs2a1;
elseif out.n_bad > 0
    ais.Xa = out.Xa1;
    ais.lnw = out.lnw1;
    ais.fs2a = out.fs2a1;
    [ais,ok] = vbmc_hip_importance_sample(ais,gp,acqfun,options,out.LB,out.UB);
    return;
else
    ais.Xa = Xa;
    ais.lnw = lnw;
    ais.fs2a = fs2a;
end
vbmc_hip_is_handle(h,ais,false,his);
ok = true;
end
