function [ais,ok] = vbmc_hip_importance_sample(ais_step1,gp,acqfun,options,LB,UB)
%VBMC_HIP_IMPORTANCE_SAMPLE Step 2 of private/activeimportancesampling_vbmc.m (:153-235) on an MI355X for acqimiqr_vbmc: the MCMC per
%   GP hyper-sample that produces the importance points, the whole sampler on the device ('acq_is_sample': vbmc_acq_is_sample).
%
%   [ais,ok] = vbmc_hip_importance_sample(ais_step1,gp,acqfun,options,LB,UB)
%
% stands where the loop over the GP hyper-samples stands, with the struct of Step 1 (Xa, lnw) and the box of :25-28.  The starting
% walkers are what :205-214 makes them: per hyper-sample W = 2(D+1) of the Step 1 points, drawn without replacement with weights
% exp(lnw + islogf2).  The transition operator is the library's ensemble slice sampler, which stands in for eissample_lite.m.  The
% struct comes back with Xa (Nm x D x S), lnw (S x Nm) and fs2a (Nm x S) filled and its device state registered with
% vbmc_hip_is_handle, so that the acquisition calls of this active-sampling step upload nothing.
%
% Given the variational posterior in place of the struct of Step 1 -- vbmc_hip_importance_sample(vp,gp,acqfun,options) -- Step 1 and the
% resampling run on the device too, in the same call (vbmc_hip_importance_setup, 'is_setup').
%
% ok = false (the caller runs its own loop): an acquisition function other than acqimiqr_vbmc, importance_sampling_vp, no MCMC samples
% requested, an unsupported GP model, or a 'vbmc_hip:unsupported' answer of the library.
ais = ais_step1;
ok = false;
if isfield(ais_step1,'mu') && ~isfield(ais_step1,'Xa')       % the variational posterior: the one-call form
    [ais,ok] = vbmc_hip_importance_setup(ais_step1,gp,acqfun,options);
    return;
end
nsamples = options.ActiveImportanceSamplingMCMCSamples;
info = acqfun('info');
supported = strcmp(func2str(acqfun),'acqimiqr_vbmc') && nsamples > 0 ...
    && ~(isfield(info,'importance_sampling_vp') && info.importance_sampling_vp) ...
    && gp.covfun(1) == 1 && any(gp.meanfun == [0 1 4]) && ~(isfield(gp,'intmeanfun') && gp.intmeanfun > 0) ...
    && ~(isfield(gp,'outwarpfun') && ~isempty(gp.outwarpfun)) && gp.noisefun(3) == 0;
if ~supported; return; end
D = size(gp.X,2);
S = numel(gp.post);
nwalkers = 2*(D+1);
[~,~,fmu,fs2] = gplite_pred(gp,ais_step1.Xa,[],[],1,0);     % every hyper-sample's prediction at the Step 1 points in one call
start = zeros(nwalkers,D,S);
for s = 1:S
    logweight = ais_step1.lnw(s,:) + acqfun('islogf2',[],[],[],fmu(:,s),fs2(:,s))';
    weight = exp(logweight - max(logweight));
    for k = 1:nwalkers
        if ~(sum(weight) > 0); weight(:) = 1; end
        steps = cumsum(weight);
        pick = find(steps > rand()*sum(weight),1);
        if isempty(pick); pick = numel(weight); end
        weight(pick) = 0;
        start(k,:,s) = min(max(ais_step1.Xa(pick,:),LB(:)'),UB(:)');
    end
end
opts = struct('Thin',options.ActiveImportanceSamplingMCMCThin,'Burnin',-1,'Spec',0,'Seed',randi(2^31-1),'Chunk',0);
h = vbmc_hip_gp_handle(gp);
try
    [Xa,lnw,fs2a,his] = vbmc_hip_mex('acq_is_sample',h,start,LB(:),UB(:),nsamples,opts);
catch err
    if ~strcmp(err.identifier,'vbmc_hip:unsupported'); rethrow(err); end
    return;
end
ais.Xa = Xa;
ais.lnw = lnw;
ais.fs2a = fs2a;
vbmc_hip_is_handle(h,ais,false,his);
ok = true;
end
