function [mtv,xx1,xx2] = vbmc_hip_mtv(vp1,vp2,Ns)
%VBMC_HIP_MTV vbmc_mtv on an MI355X ('vp_mtv': vbmc_vp_mtv), with the reference's inputs and outputs in its order.
%
%   [mtv,xx1,xx2] = vbmc_hip_mtv(vp1,vp2,Ns)
%
% The marginal total variation distances between two variational posteriors from Ns draws each: drawn, binned, smoothed by the
% diffusion estimator of shared/kde1d.m and integrated on the device (vbmc_mtv.m:24-79).  The random numbers are the library's, keyed
% by one randi of MATLAB's stream.
%
% Stays with the reference function: vp1 or vp2 given as a sample matrix, a dimension whose bandwidth equation has no bracket (the
% fminbnd branch of kde1d.m, a few dozen draws at the most) and every other 'vbmc_hip:unsupported' answer of the library.
if nargin < 3 || isempty(Ns); Ns = 1e5; end
if ~isstruct(vp1) || ~isstruct(vp2)
    [mtv,xx1,xx2] = vbmc_hip_mtv_reference(vp1,vp2,Ns,nargout);
    return;
end
try
    if nargout > 2
        [mtv,xx1,xx2] = vbmc_hip_mex('vp_mtv',vp1,vp2,Ns,randi(2^31-1));
    elseif nargout > 1
        [mtv,xx1] = vbmc_hip_mex('vp_mtv',vp1,vp2,Ns,randi(2^31-1));
    else
        mtv = vbmc_hip_mex('vp_mtv',vp1,vp2,Ns,randi(2^31-1));
    end
catch err
    if ~strcmp(err.identifier,'vbmc_hip:unsupported'); rethrow(err); end
    [mtv,xx1,xx2] = vbmc_hip_mtv_reference(vp1,vp2,Ns,nargout);
end
end

function [mtv,xx1,xx2] = vbmc_hip_mtv_reference(vp1,vp2,Ns,nout)
xx1 = [];
xx2 = [];
if nout > 1
    [mtv,xx1,xx2] = vbmc_mtv(vp1,vp2,Ns);
else
    mtv = vbmc_mtv(vp1,vp2,Ns);
end
end
