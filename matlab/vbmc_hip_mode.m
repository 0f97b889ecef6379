function [x,vp] = vbmc_hip_mode(vp,nmax,origflag)
%VBMC_HIP_MODE vbmc_mode on an MI355X ('vp_mode': vbmc_vp_mode), with the reference's inputs and outputs in its order.
%
%   [x,vp] = vbmc_hip_mode(vp,nmax,origflag)
%
% The mode of the variational posterior, in the original space (origflag, the default) or in the transformed one: the optimisation
% from up to nmax (default 20) component means runs on the device in one call.  With origflag a stored vp.mode is returned as it is,
% and the second output carries the mode in vp.mode (vbmc_mode.m:18-19, :53-55).
%
% The optimiser is the library's own (BFGS on the smooth objective in the transformed space, stopped at a gradient of 1e-6, the
% OptimalityTolerance of fminunc), not fmincon: where several local maxima tie closely the answer can be another of them, which is why
% no function named vbmc_mode is provided.  Three differences are intended: with origflag the starts are ranked by the objective at
% the starts themselves (vbmc_mode.m:24 evaluates the original-space density at transformed-space coordinates); the answer is kept
% eps, not sqrt(eps), from the bounds; a start whose density underflows is still optimised.
%
% Stays with the reference function: transform types other than 0 .. 3 and every other 'vbmc_hip:unsupported' answer of the library.
if nargin < 2 || isempty(nmax); nmax = 20; end
if nargin < 3 || isempty(origflag); origflag = true; end
if origflag && isfield(vp,'mode') && ~isempty(vp.mode)
    x = vp.mode;
    return;
end
try
    x = vbmc_hip_mex('vp_mode',vp,nmax,origflag,1e-6);
catch err
    if ~strcmp(err.identifier,'vbmc_hip:unsupported'); rethrow(err); end
    x = vbmc_mode(vp,nmax,origflag);
end
if nargout > 1 && origflag
    vp.mode = x;
end
end
