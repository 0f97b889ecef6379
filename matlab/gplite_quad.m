function [F,varF] = gplite_quad(gp,mu,sigma,ssflag)
%GPLITE_QUAD Drop-in shim: Bayesian quadrature for a GP on an MI355X through vbmc_hip_mex.
%
% Same signature and defaulting as the reference (gplite/gplite_quad.m:1-4).  The accelerated path covers the form every
% caller in VBMC uses: SE-ARD covariance, mean functions 0/1/4, constant noise, and ONE row SIGMA shared by all the points
% (a 1 x D row, or an NSTAR x D matrix whose rows are all equal).  Every other call form -- a sigma row per point, the
% squared-exponential mean functions 6/8, other noise models -- goes to the reference further down the path.
if nargin < 4 || isempty(ssflag); ssflag = false; end

Nstar = size(mu,1);
shared = size(sigma,1) == 1 || (size(sigma,1) == Nstar && all(all(bsxfun(@eq,sigma,sigma(1,:)))));
supported = shared && any(gp.meanfun == [0 1 4]) && gp.covfun(1) == 1 && isequal(gp.noisefun(:)',[1 0 0]) ...
    && ~(isfield(gp,'intmeanfun') && gp.intmeanfun > 0) && ~isempty(gp.post(1).alpha);
if supported
    try
        h = vbmc_hip_gp_handle(gp);
        if nargout > 1
            [F,varF] = vbmc_hip_mex('gp_quad',h,mu,sigma(1,:),double(ssflag),numel(gp.post));
        else
            F = vbmc_hip_mex('gp_quad',h,mu,sigma(1,:),double(ssflag),numel(gp.post));
        end
        return;
    catch err
        if ~strcmp(err.identifier,'vbmc_hip:unsupported'); rethrow(err); end
    end
end
ref = vbmc_hip_reference('gplite_quad');
if nargout > 1
    [F,varF] = ref(gp,mu,sigma,ssflag);
else
    F = ref(gp,mu,sigma,ssflag);
end
end
