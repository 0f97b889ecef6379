function [xmin,fmin,counteval,stopflag,out,bestever] = vbmc_hip_acqsearch(fitfun,xstart,insigma,inopts,vp,gp,optimState,transpose_flag,acqFun,acqInfo)
%VBMC_HIP_ACQSEARCH The acquisition search of active sampling on an MI355X: stands where private/activesample_vbmc.m:282-283 calls
%   cmaes_modded('acqwrapper_vbmc',x0(:),insigma,cmaes_opts,vp,gp,optimState,1,SearchAcqFcn{idxAcq},optimState.acqInfo{idxAcq}).
%
% Same inputs, and the outputs that call site reads: XMIN / FMIN the last generation's best point (column) and value, OUT.evals,
% BESTEVER.x / BESTEVER.f (COUNTEVAL = OUT.evals; STOPFLAG a one-cell list with the name of the stopping rule).  The whole optimiser --
% a plain (mu/mu_w,lambda)-CMA-ES in its Cholesky form inside the box inopts.LBounds / inopts.UBounds, without cmaes_modded's
% restarts, active-CMA and noise handling -- runs on the device ('acq_search'); only a progress word crosses the host link.
% private/activesample_vbmc.m cannot be shadowed from outside its folder: INTEGRATION.md documents the one-line replacement.
%
% Goes to cmaes_modded itself (same arguments) for: the IQR acquisition functions, any(vp.delta > 0), integer variables, an
% unsupported GP model, an unbounded box, or a 'vbmc_hip:unsupported' answer of the library.
% A result outside the hard bounds of the original space (acq/acqwrapper_vbmc.m:49-51, which needs warpvars_vbmc and is not part of
% the device objective) comes back with the value Inf, so that the caller's test fval_optim < fval_old (:324) keeps the sweep's point.
ids = {'acqf_vbmc','acqflog_vbmc','acqus_vbmc','acqfsn2_vbmc'};
id = find(strcmp(func2str(acqFun),ids),1) - 1;
D = numel(xstart);
quad = isfield(vp,'delta') && ~isempty(vp.delta) && any(vp.delta > 0);
boxed = isfield(inopts,'LBounds') && isfield(inopts,'UBounds') && numel(inopts.LBounds) == D && numel(inopts.UBounds) == D ...
    && all(isfinite(inopts.LBounds(:))) && all(isfinite(inopts.UBounds(:)));
supported = ~isempty(id) && ~quad && boxed && strcmp(fitfun,'acqwrapper_vbmc') && isequal(transpose_flag,1) ...
    && ~(isfield(optimState,'integervars') && any(optimState.integervars)) ...
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
        if id == 3
            [xmin,fmin,res] = vbmc_hip_mex('acq_search',h,id,vp,optimState.ymax,double(optimState.VarianceRegularizedAcqFcn), ...
                optimState.TolGPVar,xstart(:),sig,inopts.LBounds(:),inopts.UBounds(:),opts,optimState.gplengthscale,gp.X_rescaled,gp.sn2new);
        else
            [xmin,fmin,res] = vbmc_hip_mex('acq_search',h,id,vp,optimState.ymax,double(optimState.VarianceRegularizedAcqFcn), ...
                optimState.TolGPVar,xstart(:),sig,inopts.LBounds(:),inopts.UBounds(:),opts);
        end
    catch err
        if ~strcmp(err.identifier,'vbmc_hip:unsupported'); rethrow(err); end
        supported = false;
    end
end
if ~supported
    [xmin,fmin,counteval,stopflag,out,bestever] = cmaes_modded(fitfun,xstart,insigma,inopts,vp,gp,optimState,transpose_flag,acqFun,acqInfo);
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
