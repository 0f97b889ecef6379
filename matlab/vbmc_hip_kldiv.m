function [kls,xx1,xx2] = vbmc_hip_kldiv(vp1,vp2,Ns,gaussflag)
%VBMC_HIP_KLDIV vbmc_kldiv on an MI355X ('vp_kldiv': vbmc_vp_kldiv), with the reference's inputs and outputs in its order.
%
%   [kls,xx1,xx2] = vbmc_hip_kldiv(vp1,vp2,Ns,gaussflag)
%
% The two Kullback-Leibler divergences between two variational posteriors from Ns draws each, drawn, evaluated under both posteriors
% and averaged on the device (vbmc_kldiv.m:70-88).  The random numbers are the library's, keyed by one randi of MATLAB's stream.
%
% Stays with the reference function: the Gaussianized divergence (gaussflag = 1: two vbmc_moments -- vbmc_hip_moments where the
% caller wants them on the device -- and a D x D mvnkl), vp1 or vp2 given as a sample matrix, posteriors of unequal bounds and every
% other 'vbmc_hip:unsupported' answer of the library.
if nargin < 3 || isempty(Ns); Ns = 1e5; end
if nargin < 4 || isempty(gaussflag); gaussflag = false; end
if gaussflag || ~isstruct(vp1) || ~isstruct(vp2)
    [kls,xx1,xx2] = vbmc_hip_kldiv_reference(vp1,vp2,Ns,gaussflag,nargout);
    return;
end
try
    if nargout > 2
        [kls,xx1,xx2] = vbmc_hip_mex('vp_kldiv',vp1,vp2,Ns,randi(2^31-1));
    elseif nargout > 1
        [kls,xx1] = vbmc_hip_mex('vp_kldiv',vp1,vp2,Ns,randi(2^31-1));
    else
        kls = vbmc_hip_mex('vp_kldiv',vp1,vp2,Ns,randi(2^31-1));
    end
catch err
    if ~strcmp(err.identifier,'vbmc_hip:unsupported'); rethrow(err); end
    [kls,xx1,xx2] = vbmc_hip_kldiv_reference(vp1,vp2,Ns,gaussflag,nargout);
end
end

function [kls,xx1,xx2] = vbmc_hip_kldiv_reference(vp1,vp2,Ns,gaussflag,nout)
xx1 = [];
xx2 = [];
if nout > 1
    [kls,xx1,xx2] = vbmc_kldiv(vp1,vp2,Ns,gaussflag);
else
    kls = vbmc_kldiv(vp1,vp2,Ns,gaussflag);
end
end
