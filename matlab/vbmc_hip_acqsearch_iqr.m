function [xmin,fmin,counteval,stopflag,out,bestever] = vbmc_hip_acqsearch_iqr(fitfun,xstart,insigma,inopts,vp,gp,optimState,transpose_flag,acqFun,acqInfo)
%VBMC_HIP_ACQSEARCH_IQR The acquisition search of active sampling on noisy targets on an MI355X: stands where
%   private/activesample_vbmc.m:282-283 calls cmaes_modded('acqwrapper_vbmc',...) when the search function is acqviqr_vbmc or
%   acqimiqr_vbmc (misc/setupoptions_vbmc.m:144-159).
%
% Signature and outputs of vbmc_hip_acqsearch.  The optimiser is the same one ('acq_search_iqr': the Cholesky-CMA-ES on the device);
% the objective is acqwrapper_vbmc with the IQR function on optimState.ActiveImportanceSampling, whose device copy is the one the
% sweep's shim (matlab/acqwrapper_vbmc.m, 'acq_iqr') already holds.
%
% Goes to vbmc_hip_acqsearch (same arguments: the density-based functions on the device, everything else to cmaes_modded) for any other
% acquisition function, any(vp.delta > 0), integer variables, an unsupported GP model, an unbounded box, a missing
% optimState.ActiveImportanceSampling, or a 'vbmc_hip:unsupported' answer of the library.
% A result outside the hard bounds of the original space comes back with the value Inf, as in vbmc_hip_acqsearch.
ids = {'acqviqr_vbmc','acqimiqr_vbmc'};
id = find(strcmp(func2str(acqFun),ids),1) + 9;
D = numel(xstart);
quad = isfield(vp,'delta') && ~isempty(vp.delta) && any(vp.delta > 0);
boxed = isfield(inopts,'LBounds') && isfield(inopts,'UBounds') && numel(inopts.LBounds) == D && numel(inopts.UBounds) == D ...
    && all(isfinite(inopts.LBounds(:))) && all(isfinite(inopts.UBounds(:)));
supported = ~isempty(id) && ~quad && boxed && strcmp(fitfun,'acqwrapper_vbmc') && isequal(transpose_flag,1) ...
    && ~(isfield(optimState,'integervars') && any(optimState.integervars)) ...
    && isfield(optimState,'ActiveImportanceSampling') && ~isempty(optimState.ActiveImportanceSampling) ...
    && gp.covfun(1) == 1 && any(gp.meanfun == [0 1 4]) && ~(isfield(gp,'intmeanfun') && gp.intmeanfun > 0) ...
    && ~(isfield(gp,'outwarpfun') && ~isempty(gp.outwarpfun)) && gp.noisefun(3) == 0;
if supported
    opts = struct('TolX',cmaes_number(inopts,'TolX',1e-11*max(insigma),insigma), ...
        'TolFun',cmaes_number(inopts,'TolFun',1e-12,insigma),'TolHistFun',cmaes_number(inopts,'TolHistFun',1e-13,insigma), ...
        'MaxFunEvals',cmaes_number(inopts,'MaxFunEvals',Inf,insigma),'MaxIter',0,'PopSize',0,'Seed',randi(2^31-1),'Chunk',0);
    if ~isfinite(opts.MaxFunEvals); opts.MaxFunEvals = 0; end
    sig = insigma(:).*ones(D,1);
    h = vbmc_hip_gp_handle(gp);
    try
        his = vbmc_hip_is_handle(h,optimState.ActiveImportanceSampling,id == 10);
        [xmin,fmin,res] = vbmc_hip_mex('acq_search_iqr',h,his,id,vp,double(optimState.VarianceRegularizedAcqFcn), ...
            optimState.TolGPVar,xstart(:),sig,inopts.LBounds(:),inopts.UBounds(:),opts,optimState.gplengthscale,gp.X_rescaled,gp.sn2new);
    catch err
        if ~strcmp(err.identifier,'vbmc_hip:unsupported'); rethrow(err); end
        supported = false;
    end
end
if ~supported
    [xmin,fmin,counteval,stopflag,out,bestever] = vbmc_hip_acqsearch(fitfun,xstart,insigma,inopts,vp,gp,optimState,transpose_flag,acqFun,acqInfo);
    return;
end
names = {'tolx','tolfun','tolhistfun','maxfunevals','maxiter'};
counteval = res.evals;
stopflag = names(max(1,min(5,res.stop)));
out = struct('evals',res.evals,'generations',res.generations,'sigma',res.sigma,'xmean',res.xmean,'C',res.C,'behind',res.behind);
bestever = struct('x',res.xbest,'f',res.fbest,'evals',res.evals);
fmin = outside_is_inf(xmin,fmin,vp,optimState);
bestever.f = outside_is_inf(bestever.x,bestever.f,vp,optimState);
end

function v = cmaes_number(inopts,name,dflt,insigma) %#ok<INUSD>
% a numeric option of cmaes_modded, which also admits strings in terms of insigma ('1e-11*max(insigma)')
v = dflt;
if isfield(inopts,name) && ~isempty(inopts.(name))
    v = inopts.(name);
    if ischar(v); v = eval(v); end
end
end

function f = outside_is_inf(x,f,vp,optimState)
X_orig = warpvars_vbmc(x(:)','i',vp.trinfo);
if any(X_orig < optimState.LBeps_orig) || any(X_orig > optimState.UBeps_orig); f = Inf; end
end
