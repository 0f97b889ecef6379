function [X,I] = vbmc_hip_rnd(vp,N,origflag,balanceflag,df)
%VBMC_HIP_RND vbmc_rnd on an MI355X ('vp_rnd': vbmc_vp_rnd), with the reference's inputs and outputs in the reference's order.
%
%   [X,I] = vbmc_hip_rnd(vp,N,origflag,balanceflag,df)
%
% N draws from the variational posterior, in the original space through the inverse variable transform of vp.trinfo (types 0-3,
% scale, rotation) with its clamp into the bounds, or in the transformed space; balanceflag = 1 is the exact split by mixture weight.
% The random numbers are the library's, keyed by one randi of MATLAB's stream.  Deliberately not named vbmc_rnd: a same-named shim
% would intercept the one-point draws inside activesample_vbmc; the call sites with many draws choose this one (vbmc.m:1097).
%
% Falls through to the reference function for balanceflag = 'gp' and on a 'vbmc_hip:unsupported' answer of the library (a finite df,
% other transform types, D or K beyond the limits).
if nargin < 3 || isempty(origflag); origflag = true; end
if nargin < 4 || isempty(balanceflag); balanceflag = false; end
if nargin < 5 || isempty(df); df = Inf; end
if ischar(balanceflag)
    [X,I] = vbmc_hip_rnd_reference(vp,N,origflag,balanceflag,df,nargout);
    return;
end
try
    [X,I] = vbmc_hip_mex('vp_rnd',vp,N,origflag,balanceflag,df,randi(2^31-1));
    I = I + 1;
catch err
    if ~strcmp(err.identifier,'vbmc_hip:unsupported'); rethrow(err); end
    [X,I] = vbmc_hip_rnd_reference(vp,N,origflag,balanceflag,df,nargout);
end
end

function [X,I] = vbmc_hip_rnd_reference(vp,N,origflag,balanceflag,df,nout)
I = [];
if nout > 1
    [X,I] = vbmc_rnd(vp,N,origflag,balanceflag,df);
else
    X = vbmc_rnd(vp,N,origflag,balanceflag,df);
end
end
