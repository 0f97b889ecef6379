function [mubar,Sigma] = vbmc_hip_moments(vp,origflag,Ns)
%VBMC_HIP_MOMENTS vbmc_moments on an MI355X ('vp_moments': vbmc_vp_moments), with the reference's inputs and outputs in its order.
%
%   [mubar,Sigma] = vbmc_hip_moments(vp,origflag,Ns)
%
% Mean and covariance of the variational posterior in the original space from Ns balanced draws that never leave the device.  The
% random numbers are the library's, keyed by one randi of MATLAB's stream.  The transformed space (origflag = 0) is analytic and stays
% with the reference function, as does a 'vbmc_hip:unsupported' answer of the library.
if nargin < 2 || isempty(origflag); origflag = true; end
if nargin < 3 || isempty(Ns); Ns = 1e6; end
if ~origflag
    [mubar,Sigma] = vbmc_hip_moments_reference(vp,origflag,Ns,nargout);
    return;
end
try
    if nargout > 1
        [mubar,Sigma] = vbmc_hip_mex('vp_moments',vp,Ns,randi(2^31-1));
    else
        mubar = vbmc_hip_mex('vp_moments',vp,Ns,randi(2^31-1));
    end
catch err
    if ~strcmp(err.identifier,'vbmc_hip:unsupported'); rethrow(err); end
    [mubar,Sigma] = vbmc_hip_moments_reference(vp,origflag,Ns,nargout);
end
end

function [mubar,Sigma] = vbmc_hip_moments_reference(vp,origflag,Ns,nout)
Sigma = [];
if nout > 1
    [mubar,Sigma] = vbmc_moments(vp,origflag,Ns);
else
    mubar = vbmc_moments(vp,origflag,Ns);
end
end
