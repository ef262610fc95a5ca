"""``cNMF.clustergram = "device"``: consensus(show_clustering=True) orders the kept spectra on the device and writes the
clustergram picture; left at ``None`` nothing changes.  A small run: 300 cells x 120 genes, K = 4, 8 restarts."""
import glob
import os

import numpy as np
import pytest

from cnmf_amd import synth
from cnmf_amd.cnmf import cNMF

pytestmark = pytest.mark.gpu

PNG = b"\x89PNG\r\n\x1a\n"


def result_files(obj):
    """The files consensus(4, 0.5) writes (tables and text), by name relative to the run's directory: the bytes of a text
    file; of an .npz -- a zip container whose member headers carry the wall-clock time of the write -- the dtype, shape
    and bytes of every member."""
    root = os.path.join(obj.output_dir, obj.name)
    out = {}
    for f in glob.glob(os.path.join(root, "**", "*k_4.dt_0_5*"), recursive=True):
        if f.endswith(".npz"):
            with np.load(f, allow_pickle=True) as z:
                out[os.path.relpath(f, root)] = [(n, str(z[n].dtype), z[n].shape, z[n].tolist() if z[n].dtype == object
                                                  else z[n].tobytes()) for n in sorted(z.files)]
        elif not f.endswith(".png"):
            out[os.path.relpath(f, root)] = open(f, "rb").read()
    return out


@pytest.fixture(scope="module")
def runs(engine, tmp_path_factory):
    """Two runs of the same pipeline, one after the other (they share the session's engine, whose resident matrix belongs
    to one object at a time): "plain" through consensus(4, 0.5) with the attribute left at None, then "device" up to
    combine -- its consensus calls are the first test's."""
    counts, _ = synth.topic_counts(300, 120, 4, 5.5, 0.4, 7)
    made = {}
    for name in ("plain", "device"):
        obj = cNMF(output_dir=str(tmp_path_factory.mktemp(name)), name="cg", engine=engine)
        obj.prepare(counts, components=[4], n_iter=8, seed=14, num_highvar_genes=80, densify=True)
        obj.factorize()
        obj.combine()
        made[name] = obj
        if name == "plain":
            assert cNMF.clustergram is None and obj.clustergram is None
            obj.consensus(4, 0.5)
            made["plain_files"] = result_files(obj)
    return made


def test_device_clustergram_writes_the_picture_and_orders_the_kept_spectra(runs, monkeypatch):
    obj = runs["device"]
    monkeypatch.setattr(obj, "clustergram", "device", raising=False)
    obj.consensus(4, 0.5, close_clustergram_fig=True)
    png = obj.paths["clustering_plot"] % (4, "0_5")
    assert os.path.basename(png) == "cg.clustering.k_4.dt_0_5.png"
    data = open(png, "rb").read()
    assert data[:8] == PNG and len(data) > 1000
    assert obj.clustergram_fig is None                                  # closed, as asked
    labels = obj.kmeans_cluster_labels.values
    order = np.asarray(obj.spectra_order)
    n_kept = int(obj.density_filter.sum())
    assert 4 <= n_kept <= len(obj.density_filter)
    assert sorted(order.tolist()) == list(range(n_kept))                # a permutation of the kept spectra ...
    assert (np.diff(labels[order]) >= 0).all()                          # ... grouped by cluster, ascending label
    assert sorted(set(labels[order].tolist())) == [1, 2, 3, 4]
    img = obj.topics_dist_ordered
    assert img.shape == (n_kept, n_kept) and (np.diag(img) == 0).all() and np.isfinite(img).all()
    first = (order.copy(), img.copy(), result_files(obj))
    os.remove(png)
    # again: the local density now comes from its cache file (the reference has no distance matrix on that branch)
    assert os.path.isfile(obj.paths["local_density_cache"] % 4)
    obj.consensus(4, 0.5)
    assert np.array_equal(obj.spectra_order, first[0])
    assert obj.topics_dist_ordered.tobytes() == first[1].tobytes()
    assert open(png, "rb").read()[:8] == PNG and obj.clustergram_fig is not None
    assert result_files(obj) == first[2]
    runs["device_files"] = first[2]


def test_attribute_left_at_none_changes_nothing(runs):
    obj = runs["plain"]
    assert not os.path.exists(obj.paths["clustering_plot"] % (4, "0_5"))
    assert not glob.glob(os.path.join(obj.output_dir, obj.name, "**", "*.png"), recursive=True)
    assert obj.topics_dist is None and not hasattr(obj, "spectra_order")
    files = runs["plain_files"]
    assert len(files) >= 9
    if "device_files" not in runs:                                       # (this test selected alone)
        dev = runs["device"]
        dev.clustergram = "device"
        dev.consensus(4, 0.5, close_clustergram_fig=True)
        runs["device_files"] = result_files(dev)
    assert sorted(files) == sorted(runs["device_files"])
    for name in files:
        assert files[name] == runs["device_files"][name], name


def test_any_other_value_is_refused(runs):
    obj = runs["plain"]
    obj.clustergram = "host"
    try:
        with pytest.raises(ValueError, match="clustergram"):
            obj.consensus(4, 0.5)
    finally:
        del obj.clustergram
