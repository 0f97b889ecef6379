function [y,dy] = vbmc_hip_pdf(vp,X,origflag,logflag,transflag,df)
%VBMC_HIP_PDF vbmc_pdf on an MI355X ('vp_pdf': vbmc_vp_pdf), with the reference's inputs and outputs in the reference's order.
%
%   [y,dy] = vbmc_hip_pdf(vp,X,origflag,logflag,transflag,df)
%
% The density of the variational posterior at the rows of X: the Gaussian mixture and both heavy-tailed variants, in the original
% space through the variable transform of vp.trinfo (types 0-3, scale, rotation) or in the transformed space.  Deliberately not named
% vbmc_pdf: the call sites choose it (vbmc.m:1119, vbmc_kldiv).
%
% Falls through to the reference function on a 'vbmc_hip:unsupported' answer of the library (other transform types, a gradient the
% device does not form, D or K beyond the limits).
if nargin < 3 || isempty(origflag); origflag = true; end
if nargin < 4 || isempty(logflag); logflag = false; end
if nargin < 5 || isempty(transflag); transflag = false; end
if nargin < 6 || isempty(df); df = Inf; end
try
    if nargout > 1
        [y,dy] = vbmc_hip_mex('vp_pdf',vp,X,origflag,logflag,transflag,df);
    else
        y = vbmc_hip_mex('vp_pdf',vp,X,origflag,logflag,transflag,df);
    end
catch err
    if ~strcmp(err.identifier,'vbmc_hip:unsupported'); rethrow(err); end
    if nargout > 1
        [y,dy] = vbmc_pdf(vp,X,origflag,logflag,transflag,df);
    else
        y = vbmc_pdf(vp,X,origflag,logflag,transflag,df);
    end
end
end
