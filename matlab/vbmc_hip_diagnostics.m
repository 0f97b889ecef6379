function [exitflag,best,idx_best,stats] = vbmc_hip_diagnostics(vp_array,beta_lcb,elbo_thresh,sKL_thresh,maxmtv_thresh,opts)
%VBMC_HIP_DIAGNOSTICS vbmc_diagnostics with every pair's divergences from one call on an MI355X ('vp_diag': vbmc_vp_diagnostics).
%
%   [exitflag,best,idx_best,stats] = vbmc_hip_diagnostics(vp_array,beta_lcb,elbo_thresh,sKL_thresh,maxmtv_thresh,opts)
%
% The reference's inputs and outputs in its order, then an options struct: opts.Ns (draws per run, 1e5), opts.Seed (the key of the
% library's draws; one randi of MATLAB's stream if absent) and opts.Display (true).  Exit flags: 1 passed; 0 one converged run;
% -1 too few runs agree with the best posterior; -2 too few agree with the best ELBO; -3 no run converged.
%
% This is not a same-named replacement of vbmc_diagnostics: the draws are the library's, and run i is drawn ONCE and meets every
% other run on those draws, where the reference draws afresh for each pair.  Two more differences, both on purpose:
%   * vbmc_diagnostics.m:53-56 compare nargin with a number one too high, so the reference replaces the last argument a caller gives
%     by its default.  Here an argument that is given is used, as the reference's help text says.
%   * as in the reference, the largest marginal total variation of a pair skips dimensions that are NaN.
%
% Stays with the reference function: more than 32 runs, a dimension whose bandwidth equation has no bracket, and every other
% 'vbmc_hip:unsupported' answer of the library.  (There the reference's own reading of its arguments applies: it takes five, and
% its fifth, maxmtv_thresh, is the one its defaults overwrite.)
if nargin < 2 || isempty(beta_lcb); beta_lcb = 3; end
if nargin < 3 || isempty(elbo_thresh); elbo_thresh = 1; end
if nargin < 4 || isempty(sKL_thresh); sKL_thresh = 1; end
if nargin < 5 || isempty(maxmtv_thresh); maxmtv_thresh = 0.2; end
if nargin < 6 || isempty(opts); opts = struct(); end
Ns = 1e5;
if isfield(opts,'Ns') && ~isempty(opts.Ns); Ns = opts.Ns; end
show = true;
if isfield(opts,'Display') && ~isempty(opts.Display); show = opts.Display; end
if isfield(opts,'Seed') && ~isempty(opts.Seed); seed = opts.Seed; else; seed = randi(2^31-1); end
if isstruct(vp_array); vp_array = num2cell(vp_array); end
Nruns = numel(vp_array);

kl_mat = zeros(Nruns,Nruns);
maxmtv_mat = zeros(Nruns,Nruns);
if Nruns > 1
    try
        [kl_mat,maxmtv_mat] = vbmc_hip_mex('vp_diag',Ns,seed,vp_array{:});
    catch err
        if ~strcmp(err.identifier,'vbmc_hip:unsupported'); rethrow(err); end
        if nargout > 3
            [exitflag,best,idx_best,stats] = vbmc_diagnostics(vp_array,beta_lcb,elbo_thresh,sKL_thresh,maxmtv_thresh);
        else
            [exitflag,best,idx_best] = vbmc_diagnostics(vp_array,beta_lcb,elbo_thresh,sKL_thresh,maxmtv_thresh);
            stats = [];
        end
        return;
    end
else
    warning('vbmc_hip_diagnostics:SingleInput','The diagnostics compare several runs; one run cannot be compared with anything.');
end

elbo = NaN(1,Nruns); elbo_sd = NaN(1,Nruns); stable = false(1,Nruns);
for i = 1:Nruns
    elbo(i) = vp_array{i}.stats.elbo;
    elbo_sd(i) = vp_array{i}.stats.elbo_sd;
    stable(i) = vp_array{i}.stats.stable;
end
exitflag = Inf;
active = stable;
if ~any(stable)
    warning('vbmc_hip_diagnostics:NoneConverged','No run has converged; the comparisons use a solution that may be unstable.');
    active = true(1,Nruns);
    exitflag = -3;
elseif nnz(stable) == 1
    warning('vbmc_hip_diagnostics:OneConverged','Only one run has converged; perform more runs.');
    exitflag = 0;
end
elcbo = elbo - beta_lcb*elbo_sd;
score = elcbo;
score(~active) = -Inf;
[~,ibest] = max(score);
sKL_best = 0.5*(kl_mat(:,ibest)' + kl_mat(ibest,:));
maxmtv_best = maxmtv_mat(ibest,:);
if Nruns > 1
    need = max(Nruns/3,2);
    if nnz(abs(elbo(ibest) - elbo) < elbo_thresh) < need; exitflag = min(exitflag,-2); end
    if nnz(sKL_best < sKL_thresh) < need; exitflag = min(exitflag,-1); end
    if nnz(maxmtv_best < maxmtv_thresh) < need; exitflag = min(exitflag,-1); end
end
if isinf(exitflag); exitflag = 1; end
texts = {'no run has converged','too few runs agree with the best ELBO', ...
    'too few runs agree with the best posterior (symmetrized KL divergence or largest marginal total variation)', ...
    'only one run has converged','passed'};
msg = ['Diagnostics: ' texts{exitflag + 4} '.'];
if show
    fprintf('%d of %d runs have converged.\n',nnz(stable),Nruns);
    for i = 1:Nruns
        fprintf('%4d  elbo %10.2f  sd %8.2f  elcbo %10.2f  converged %d  sKL %9.2f  maxMTV %6.2f%s\n', ...
            i,elbo(i),elbo_sd(i),elcbo(i),stable(i),sKL_best(i),maxmtv_best(i),repmat(' <- best',1,double(i == ibest)));
    end
    fprintf('%s\n',msg);
end
if stable(ibest)
    idx_best = ibest;
    best = struct('vp',vp_array{ibest},'elbo',elbo(ibest),'elbo_sd',elbo_sd(ibest));
else
    idx_best = [];
    best = [];
end
stats = struct('beta_lcb',beta_lcb,'elbo_thresh',elbo_thresh,'sKL_thresh',sKL_thresh,'maxmtv_thresh',maxmtv_thresh, ...
    'elbo',elbo,'elbo_sd',elbo_sd,'elcbo',elcbo,'idx_best',idx_best,'sKL_best',sKL_best,'maxmtv_best',maxmtv_best, ...
    'kl_mat',kl_mat,'maxmtv_mat',maxmtv_mat,'exitflag',exitflag,'msg',msg);
end
