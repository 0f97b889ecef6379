function [S,ok] = vbmc_hip_cornerdata(src,names,truths,bounds,Ns,balanceflag)
%VBMC_HIP_CORNERDATA The numbers of a corner plot on an MI355X ('vp_corner': vbmc_vp_corner).
%
%   [S,ok] = vbmc_hip_cornerdata(vp)                         what vbmc_plot(vp) hands to cornerplot and what that computes
%   [S,ok] = vbmc_hip_cornerdata(vp,names,truths,bounds,Ns,balanceflag)
%   [S,ok] = vbmc_hip_cornerdata(X,names,truths,bounds)      for the rows of a sample matrix, as cornerplot(X,names,truths,bounds)
%
% src is a variational posterior (Ns draws, default 1e5 as in vbmc_plot.m; balanceflag 1 is vbmc_iterplot's draw) or a matrix with one
% sample per row.  names, truths and bounds (2 x D, first row the lower bounds; empty or all zero: each column's min and max) are
% cornerplot's and travel on in S for the drawing.  The random numbers are the library's, keyed by one randi of MATLAB's stream.
%
% S.ok, S.xx (Ns x D), S.bounds (2 x D, the ones used), S.hist (40 x D counts on 40 equal bins between the bounds: the probability
% is the count over the number of rows; MATLAB's histogram picks "nice" edges of its own), S.median (1 x D), S.density (64 x 64 x P,
% page pp what kde2d returns for the pp-th pair d1 < d2 in cornerplot's order, on the mesh of 64 points between the bounds of d1
% (columns) and d2 (rows)), S.bandwidth (2 x P), S.names, S.truths.
%
% ok is false, and S holds the library's message, where the library answers 'vbmc_hip:unsupported' (a pair that reaches kde2d's
% fminbnd branch, transform types 4 .. 13, more than 32 dimensions): the caller then draws with the reference's functions.
if nargin < 2; names = {}; end
if nargin < 3; truths = []; end
if nargin < 4; bounds = []; end
if nargin < 5 || isempty(Ns); Ns = 1e5; end
if nargin < 6 || isempty(balanceflag); balanceflag = 0; end
if ~isempty(bounds) && all(bounds(:) == 0); bounds = []; end
ok = false;
seed = randi(2^31-1);
try
    if isstruct(src)
        [xx,b,h,q,dens,bw] = vbmc_hip_mex('vp_corner',src,[],Ns,seed,balanceflag,bounds,0,0,0.5);
    else
        [xx,b,h,q,dens,bw] = vbmc_hip_mex('vp_corner',[],src,0,seed,0,bounds,0,0,0.5);
    end
catch err
    if ~strcmp(err.identifier,'vbmc_hip:unsupported'); rethrow(err); end
    S = struct('ok',false,'message',err.message);
    return;
end
ok = true;
S = struct('ok',true,'xx',xx,'bounds',b,'hist',h,'median',q,'density',dens,'bandwidth',bw,'names',{names},'truths',truths);
end
