function vbmc_hip_plot(vp_array,stats)
%VBMC_HIP_PLOT vbmc_plot with the numbers computed on an MI355X (vbmc_hip_cornerdata: 'vp_corner').
%
%   vbmc_hip_plot(vp)                 the corner plot of one variational posterior
%   vbmc_hip_plot(vp_array,stats)     the marginals and medians of several (a cell array), the best one of stats.idx_best in bold
%
% Stands where vbmc_plot(vp_array,stats) stands.  The draws, the histograms, the pair densities and the medians come from the
% device; this file only builds the meshes from the bounds and draws: stairs for the histograms, contour(X,Y,density,10) for the
% pairs.  The histograms show counts on 40 equal bins between the bounds (the reference shows count / Ns on histogram's own "nice"
% edges: the same shape; the corner plot hides those ticks).
%
% Goes to the reference's vbmc_plot: an entry that is not a variational posterior, and every posterior on which
% vbmc_hip_cornerdata reports ok = false.
if nargin < 2; stats = []; end
if ~iscell(vp_array); vp_array = {vp_array}; end
Nvps = numel(vp_array);
S = cell(1,Nvps);
for i = 1:Nvps
    if ~isstruct(vp_array{i}); vbmc_plot(vp_array,stats); return; end
    [S{i},ok] = vbmc_hip_cornerdata(vp_array{i});
    if ~ok; vbmc_plot(vp_array,stats); return; end
end
if Nvps == 1
    D = size(S{1}.bounds,2);
    names = cell(1,D);
    for d = 1:D; names{d} = ['x_{' num2str(d) '}']; end
    S{1}.names = names;
    draw_corner(S{1});
else
    draw_marginals(S,stats);
end
end

function draw_corner(S)
D = size(S.bounds,2);
res = size(S.density,1);
figure;
set(gcf,'Color','w');
for d = 1:D
    subplot(D,D,(d-1)*D+d);
    draw_stairs(S,d,'k',1);
    set(gca,'XLim',S.bounds(:,d)','YTick',[],'TickDir','out','Box','off');
    if d < D; set(gca,'XTickLabel',[]); end
    if ~isempty(S.truths); hold on; plot([S.truths(d) S.truths(d)],ylim,'k-'); end
    if ~isempty(S.names)
        if d == 1; ylabel(S.names{d}); end
        if d == D; xlabel(S.names{d}); end
    end
end
pp = 0;
for d1 = 1:D-1
    for d2 = d1+1:D
        pp = pp + 1;
        subplot(D,D,(d2-1)*D+d1);
        [X,Y] = meshgrid(linspace(S.bounds(1,d1),S.bounds(2,d1),res),linspace(S.bounds(1,d2),S.bounds(2,d2),res));
        contour(X,Y,S.density(:,:,pp),10);
        set(gca,'XLim',S.bounds(:,d1)','YLim',S.bounds(:,d2)','TickDir','out','Box','off');
        if d1 > 1; set(gca,'YTickLabel',[]); end
        if d2 < D; set(gca,'XTickLabel',[]); end
        if ~isempty(S.truths)
            hold on;
            plot(S.bounds(:,d1)',[S.truths(d2) S.truths(d2)],'k-');
            plot([S.truths(d1) S.truths(d1)],S.bounds(:,d2)','k-');
        end
        if ~isempty(S.names)
            if d1 == 1; ylabel(S.names{d2}); end
            if d2 == D; xlabel(S.names{d1}); end
        end
    end
end
end

function draw_marginals(S,stats)
Nvps = numel(S);
D = size(S{1}.bounds,2);
ncols = ceil(sqrt(D));
nrows = ceil(D/ncols);
cmap = lines(Nvps);
hln = zeros(1,Nvps);
ltext = cell(1,Nvps);
for i = 1:Nvps
    best = ~isempty(stats) && stats.idx_best == i;
    ltext{i} = ['vp #' num2str(i)];
    if best; ltext{i} = [ltext{i} ' (best)']; end
    for d = 1:D
        subplot(nrows,ncols,d);
        draw_stairs(S{i},d,cmap(i,:),1 + 2*best);
        hold on;
    end
end
for i = 1:Nvps
    best = ~isempty(stats) && stats.idx_best == i;
    for d = 1:D
        subplot(nrows,ncols,d);
        hln(i) = plot([S{i}.median(d) S{i}.median(d)],ylim,'-','LineWidth',1 + 2*best,'Color',cmap(i,:));
    end
end
for d = 1:D
    subplot(nrows,ncols,d);
    xlabel(['x_{' num2str(d) '}']);
    set(gca,'TickDir','out','Box','off');
    if d == D
        hleg = legend(hln,ltext{:});
        set(hleg,'Box','off','Location','best');
    end
end
set(gcf,'Color','w');
end

function draw_stairs(S,d,col,lw)
nb = size(S.hist,1);
edges = linspace(S.bounds(1,d),S.bounds(2,d),nb+1);
stairs(edges,[S.hist(:,d); S.hist(nb,d)],'Color',col,'LineWidth',lw);
end
