"""The consensus clustergram as a picture: what a cNMF user reads to choose ``density_threshold``.

``save_clustergram`` draws the four things ``cNMF.consensus(show_clustering=True)`` has at hand once
``Engine.clustergram`` ordered the kept spectra on the device:

* the ordered distance matrix with its colour bar,
* the k-means label of every ordered spectrum as a strip above and to the left of the matrix,
* the histogram of the local densities of ALL spectra with the threshold marked,
* how many spectra the threshold removed.

matplotlib is imported here, lazily, with the Agg backend -- the package itself never needs it.  Without matplotlib the
arrays on the ``cNMF`` object are what remains: a ``UserWarning`` says that the picture was skipped.
"""
import warnings

import numpy as np


def save_clustergram(path, dist_ordered, labels_ordered, local_density, density_threshold, n_removed, close=False,
                     dpi=250):
    """Write the figure to ``path`` (PNG).  Returns the figure, or ``None`` when it was closed or could not be made."""
    try:
        from matplotlib.figure import Figure                              # (no pyplot: the caller's backend is left alone)
        from matplotlib.backends.backend_agg import FigureCanvasAgg
    except ImportError:
        warnings.warn("matplotlib is not installed: the clustergram picture %s was skipped "
                      "(spectra_order and topics_dist_ordered are set)" % path, UserWarning, stacklevel=2)
        return None
    dist_ordered = np.asarray(dist_ordered)
    labels_ordered = np.asarray(labels_ordered)
    local_density = np.asarray(local_density, dtype=np.float64).ravel()
    n_all, n_kept = local_density.size, labels_ordered.size

    fig = Figure(figsize=(13.5, 8.5))
    FigureCanvasAgg(fig)
    grid = fig.add_gridspec(2, 4, width_ratios=[0.35, 8, 0.6, 4], height_ratios=[0.35, 8],
                            left=0.02, right=0.97, bottom=0.03, top=0.95, wspace=0.02, hspace=0.02)
    ax_img = fig.add_subplot(grid[1, 1])
    image = ax_img.imshow(dist_ordered, cmap="viridis", aspect="auto", interpolation="none", rasterized=True)
    ax_img.set_xticks([])
    ax_img.set_yticks([])
    strip_kw = dict(cmap="Spectral", aspect="auto", interpolation="none", rasterized=True,
                    vmin=labels_ordered.min() if n_kept else 0, vmax=labels_ordered.max() if n_kept else 1)
    ax_top = fig.add_subplot(grid[0, 1])
    ax_top.imshow(labels_ordered[None, :], **strip_kw)
    ax_top.set_title("%d spectra in %d clusters, average-linkage leaf order within a cluster"
                     % (n_kept, len(np.unique(labels_ordered))), fontsize=10)
    ax_left = fig.add_subplot(grid[1, 0])
    ax_left.imshow(labels_ordered[:, None], **strip_kw)
    for ax in (ax_top, ax_left):
        ax.set_xticks([])
        ax.set_yticks([])

    side = grid[1, 3].subgridspec(3, 1, height_ratios=[5, 1.2, 6], hspace=0.9)
    ax_hist = fig.add_subplot(side[0, 0])
    upper = max(1.0, float(local_density.max()) if n_all else 1.0)
    ax_hist.hist(local_density, bins=np.linspace(0.0, upper, 50), color="0.35")
    if density_threshold <= upper:
        ax_hist.axvline(density_threshold, color="crimson", linestyle="--", linewidth=1.2)
        ax_hist.annotate("threshold %g" % density_threshold, xy=(density_threshold, 1.0), xycoords=("data", "axes fraction"),
                         xytext=(3, -3), textcoords="offset points", va="top", color="crimson", fontsize=9)
    ax_hist.set_title("Local density of all %d spectra" % n_all, fontsize=10)
    ax_hist.set_xlabel("mean distance to the nearest neighbours")
    ax_hist.set_ylabel("spectra")
    share = 100.0 * n_removed / n_all if n_all else 0.0
    ax_hist.text(0.5, -0.42, "%d of %d spectra (%.0f%%) at or above the threshold\nwere removed before clustering"
                 % (n_removed, n_all, share), transform=ax_hist.transAxes, ha="center", va="top", fontsize=9)
    ax_bar = fig.add_subplot(side[1, 0])
    fig.colorbar(image, cax=ax_bar, orientation="horizontal")
    ax_bar.set_title("Euclidean distance between L2-normalised spectra", fontsize=10)
    fig.add_subplot(side[2, 0]).set_axis_off()

    fig.savefig(path, dpi=dpi)
    if close:
        fig.clear()
        return None
    return fig
