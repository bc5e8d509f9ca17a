"""Test-set evaluation flow of the reference (crimac_unet/pipeline_train_predict/evaluate.py:39-117) on the
MI355X pipeline.

The reference's ``validate_model_survey_zarr`` / ``validate_model_survey_memm`` build a gridded Dataset over one
survey (zarr) or over every echogram of a survey (memm), wrap it in a DataLoader and hand it to
``SegPipe.validate_model_testing``.  Datasets, readers and label transforms are the reference's host-side numpy
stack (unchanged, fed through the batch-dict API); what runs on the GPU here is
``predict_batch`` (HIP U-Net) and, with ``gpu_metrics``, the PR histograms.  The two functions below keep the
reference's names, keyword arguments and file naming.  This package never reaches into the reference on its own: the
Dataset class and the transform factories are INJECTED (``dataset_cls`` / ``data_transform_factory`` /
``label_transform_factory``), and the command line (``python -m crimac_classifiers_unet_amd.evaluate``, the reference's
``evaluate.py`` ``__main__``, :120-167) takes the location of the host data stack as an explicit ``--data-stack`` path.

``tiled=True`` (``--tiled``) runs the same evaluation without that host chain: ``tiled_inference.evaluate_survey`` /
``evaluate_echograms_memm`` keep the survey chunk, the crops, the label and data transforms and the PR histograms on the
GPU and need the readers only -- no Dataset class, no transform factory, no DataLoader workers.
"""
from __future__ import annotations

import os

from torch.utils.data import ConcatDataset, DataLoader


def _reference_factories(dataset_cls, data_transform_factory, label_transform_factory, memm):
    """The host-side Dataset and transform factories must be handed in (no implicit import of another package)."""
    missing = [n for n, v in (("dataset_cls", dataset_cls), ("data_transform_factory", data_transform_factory),
                              ("label_transform_factory", label_transform_factory)) if v is None]
    if missing:
        raise ImportError(
            f"validate_model_survey_{'memm' if memm else 'zarr'}: pass {', '.join(missing)} explicitly -- the gridded "
            "Dataset class (the reference's batch.dataset.DatasetGriddedReader), the data-transform factory "
            f"(batch.transforms.{'define_data_transform_test' if memm else 'define_data_transform'}) and the "
            "label-transform factory (batch.transforms.define_label_transform_test); `data_stack_factories(path)` "
            "builds the three from an explicitly named checkout of the host data stack")
    return dataset_cls, data_transform_factory, label_transform_factory


def data_stack_factories(path, memm):
    """The three host-side factories from the data stack at ``path`` (a checkout of the reference's ``crimac_unet``
    directory, NAMED BY THE CALLER): ``(DatasetGriddedReader, data-transform factory, label-transform factory)``."""
    import importlib
    import sys
    path = os.path.abspath(str(path))
    if not os.path.isdir(os.path.join(path, "batch")):
        raise ImportError(f"{path} does not look like the host data stack (no batch/ package)")
    if path not in sys.path:
        sys.path.insert(0, path)
    ds = importlib.import_module("batch.dataset")
    tr = importlib.import_module("batch.transforms")
    return (ds.DatasetGriddedReader, tr.define_data_transform_test if memm else tr.define_data_transform,
            tr.define_label_transform_test)


def _is_use_metadata(meta_channels):
    return len(meta_channels) > 0


def validate_model_survey_zarr(readers, segpipe, meta_channels, patch_size, patch_overlap, eval_mode, batch_size,
                               num_workers, save_path_metrics, save_path_plot, preload_n_pings=0, survey="survey",
                               dataset_cls=None, data_transform_factory=None, label_transform_factory=None,
                               worker_init_fn=None, tiled=False, eval_classes=None, **kwargs):
    """evaluate.py:39-81: one zarr file = one survey; gridded patches of the whole survey -> PR curve / F1.
    ``tiled=True``: on the tiled GPU path (``tiled_inference.evaluate_survey``); ``preload_n_pings`` > 0 is then the
    chunk size (0: the default of ``predict_survey``), and no factory is needed.
    ``eval_classes`` (foreground class indices, e.g. ``(1, 2)``; ``tiled`` or the segpipe's ``gpu_metrics``): the PR
    curve / F1 of each class from the one pass -- ``{class: metrics}``, files ``{survey}_test_sandeel.csv``,
    ``{survey}_test_other.csv``, ``{survey}_pr_sandeel.png`` ..."""
    eval_classes = _eval_classes(eval_classes, tiled, segpipe)
    if tiled:
        from .tiled_inference import evaluate_survey
        if not segpipe.model_is_loaded:
            segpipe.load_model_params()
        assert len(readers) == 1, "Current evaluation code assumes one zarr file contains an entire survey"
        hp, hn = evaluate_survey(readers[0], segpipe, patch_size, patch_overlap, batch_size, preload_n_pings,
                                 eval_mode=eval_mode, classes=eval_classes)
        return _tiled_metrics(segpipe, hp, hn, save_path_metrics, save_path_plot, survey, eval_classes)
    dataset_cls, dtf, ltf = _reference_factories(dataset_cls, data_transform_factory, label_transform_factory, False)
    assert len(readers) == 1, "Current evaluation code assumes one zarr file contains an entire survey"
    assert preload_n_pings == 0, "Current evaluation code for zarr only works when 'preloading_n_pings' = 0"
    frequencies = segpipe.frequencies
    data_transform = dtf(_is_use_metadata(meta_channels))
    label_transform = ltf(frequencies=frequencies, label_masks=eval_mode, patch_overlap=patch_overlap)
    metrics = None
    for reader in readers:
        dataset = dataset_cls(reader, patch_size, frequencies, meta_channels=meta_channels, grid_start=None,
                              grid_end=None, patch_overlap=patch_overlap, data_preload=False,
                              augmentation_function=None, label_transform_function=label_transform,
                              data_transform_function=data_transform, grid_mode="all")
        dataloader = DataLoader(dataset, batch_size=batch_size, shuffle=False, num_workers=num_workers,
                                worker_init_fn=worker_init_fn)
        metrics = segpipe.validate_model_testing(
            dataloader, save_path_metrics=os.path.join(save_path_metrics, f"{survey}_test.csv"),
            save_path_plot=os.path.join(save_path_plot, f"{survey}_pr.png"), **_classes_kw(eval_classes))
    return metrics


def validate_model_survey_memm(readers, segpipe, meta_channels, patch_size, patch_overlap, eval_mode, batch_size,
                               num_workers, save_path_metrics, save_path_plot, survey="survey", dataset_cls=None,
                               data_transform_factory=None, label_transform_factory=None, worker_init_fn=None,
                               tiled=False, eval_classes=None, **kwargs):
    """evaluate.py:84-117: one gridded Dataset per echogram, concatenated -> PR curve / F1 of the survey.
    ``tiled=True``: the whole survey on the tiled GPU path (``tiled_inference.evaluate_echograms_memm``: forward batches
    packed across the echograms, one feed; with several ranks the groups of echograms are dealt to the ranks and the
    histograms all-reduced once; a model with metadata planes goes echogram by echogram unless ``pack_metadata=True`` is
    among ``kwargs``); no factory is needed.  ``eval_classes``: as ``validate_model_survey_zarr``."""
    eval_classes = _eval_classes(eval_classes, tiled, segpipe)
    if tiled:
        from .tiled_inference import evaluate_echograms_memm
        if not segpipe.model_is_loaded:
            segpipe.load_model_params()
        hp, hn = evaluate_echograms_memm(readers, segpipe, patch_size, patch_overlap, batch_size, eval_mode=eval_mode,
                                         meta_channels=meta_channels or None, classes=eval_classes,
                                         **{k: kwargs[k] for k in ("pack_metadata",) if k in kwargs})
        return _tiled_metrics(segpipe, hp, hn, save_path_metrics, save_path_plot, survey, eval_classes)
    dataset_cls, dtf, ltf = _reference_factories(dataset_cls, data_transform_factory, label_transform_factory, True)
    frequencies = segpipe.frequencies
    data_transform = dtf(_is_use_metadata(meta_channels))
    label_transform = ltf(frequencies=frequencies, label_masks=eval_mode, patch_overlap=patch_overlap)
    datasets = [dataset_cls(reader, patch_size, frequencies, meta_channels=meta_channels, grid_start=None,
                            grid_end=None, patch_overlap=patch_overlap, augmentation_function=None,
                            label_transform_function=label_transform, data_transform_function=data_transform,
                            grid_mode="all") for reader in readers]
    dataloader = DataLoader(ConcatDataset(datasets), batch_size=batch_size, shuffle=False, num_workers=num_workers,
                            worker_init_fn=worker_init_fn)
    return segpipe.validate_model_testing(
        dataloader, save_path_metrics=os.path.join(save_path_metrics, f"{survey}_test.csv"),
        save_path_plot=os.path.join(save_path_plot, f"{survey}_pr.png"), **_classes_kw(eval_classes))


def _eval_classes(eval_classes, tiled, segpipe):
    """``eval_classes`` of the two functions above -> None or a checked tuple; refused before anything is read where no
    per-class form exists: the sklearn path (neither ``tiled`` nor ``gpu_metrics``) scores the sandeel class only."""
    if eval_classes is None:
        return None
    if not (tiled or getattr(segpipe, "gpu_metrics", False)):
        raise ValueError(f"eval_classes={eval_classes!r} (--classes) needs tiled=True (--tiled) or gpu_metrics: the "
                         "per-class PR curves come from the GPU histograms, the sklearn path scores the sandeel class only")
    from .tiled_inference import check_classes
    return check_classes(eval_classes, segpipe.model.n_classes)


def _classes_kw(eval_classes):
    return {} if eval_classes is None else {"classes": eval_classes}


def parse_classes(text, n_classes=None):
    """``--classes``: ``"1,2"`` -> (1, 2); ``"all"`` -> every foreground class of an ``n_classes`` model (None: the string
    'all' is handed back for the caller to resolve once the model exists)."""
    if text is None:
        return None
    if isinstance(text, str):
        if text.strip().lower() == "all":
            return "all" if n_classes is None else tuple(range(1, n_classes))
        try:
            return tuple(int(t) for t in text.split(","))
        except ValueError:
            raise ValueError(f"--classes {text!r}: comma-separated class indices such as 1,2, or 'all'") from None
    return tuple(text)


def _tiled_metrics(segpipe, hist_pos, hist_neg, save_path_metrics, save_path_plot, survey, eval_classes=None):
    return segpipe.validate_model_testing_from_histograms(
        hist_pos, hist_neg,
        save_path_metrics=None if save_path_metrics is None else os.path.join(save_path_metrics, f"{survey}_test.csv"),
        save_path_plot=None if save_path_plot is None else os.path.join(save_path_plot, f"{survey}_pr.png"),
        **_classes_kw(eval_classes))


def main(argv=None, data_partition_factory=None, factories=None):
    """``evaluate.py`` ``__main__`` (evaluate.py:120-167): yaml + command line -> SegPipeUNet with loaded parameters ->
    for every evaluation survey of the data partition: PR curve / F1 csv + plot.

    The host data stack (readers, partition, Dataset, transforms: SURVEY.md §2 rows 5-9, out of scope here) is named
    explicitly: ``--data-stack PATH`` (a checkout of the reference's ``crimac_unet`` directory), or injected by the
    caller -- ``data_partition_factory(**config) -> object with get_evaluation_surveys() / get_survey_readers(survey)``
    and ``factories = (dataset_cls, data_transform_factory, label_transform_factory)``."""
    import argparse
    import time
    from pathlib import Path

    import yaml

    from .pipeline import SegPipeUNet
    ap = argparse.ArgumentParser(description="Test-set evaluation (PR curve, F1) of a trained U-Net on MI355X")
    ap.add_argument("--yaml_path", type=lambda p: Path(p).resolve(strict=True), required=True)
    ap.add_argument("--checkpoint_path", type=lambda p: Path(p).resolve(strict=True), required=True)
    ap.add_argument("--save_path_metrics", type=lambda p: Path(p).resolve(strict=True), required=True)
    ap.add_argument("--save_path_plot", type=lambda p: Path(p).resolve(strict=True), required=True)
    ap.add_argument("--save_model_params", action="store_true", default=False)
    ap.add_argument("--batch_size", type=int)
    ap.add_argument("--data_mode", choices=["memm", "zarr"])
    ap.add_argument("--data-stack", dest="data_stack", default=None,
                    help="checkout of the host data stack (the reference's crimac_unet directory): readers, partition, "
                         "Dataset, transforms (with --tiled: readers and partition only)")
    ap.add_argument("--tiled", action="store_true", default=None,
                    help="evaluate on the tiled GPU path: chunk, crops, transforms and PR histograms stay on the GPU; "
                         "no Dataset / transform factories, no DataLoader workers")
    ap.add_argument("--classes", dest="eval_classes", default=None,
                    help="foreground classes to score from the one pass, e.g. 1,2 ('all': every foreground class): one "
                         "csv / plot / F1 line per class (_sandeel, _other, _class{k}); needs --tiled or gpu_metrics")
    args = ap.parse_args(argv)
    config = yaml.safe_load(open(args.yaml_path))
    for k, v in vars(args).items():                     # command line takes precedence (utils/general.py:128-136)
        if v is not None or k not in config:
            config[k] = v
    data_stack = config.pop("data_stack", None)
    experiment_name = Path(config["yaml_path"]).stem
    memm = config["data_mode"] == "memm"
    if config["data_mode"] not in ("zarr", "memm"):
        raise ValueError('data_mode not in ["zarr", "memm"]')
    tiled = bool(config.pop("tiled", False))
    eval_classes = parse_classes(config.pop("eval_classes", None))
    if eval_classes is not None and not (tiled or config.get("gpu_metrics")):
        raise ValueError("--classes needs --tiled or gpu_metrics: the per-class PR curves come from the GPU histograms, the "
                         "sklearn path scores the sandeel class only")
    if tiled:
        factories = factories or (None, None, None)
    if factories is None:
        if data_stack is None:
            raise SystemExit("evaluate: name the host data stack with --data-stack PATH (or call main() with injected "
                             "factories): this package does not import it on its own")
        factories = data_stack_factories(data_stack, memm)
    if data_partition_factory is None:
        if data_stack is None:
            raise SystemExit("evaluate: --data-stack PATH is needed for the data partition (data.partition.DataZarr / DataMemm)")
        import importlib
        data_stack_factories(data_stack, memm)          # (puts the named path on sys.path)
        part = importlib.import_module("data.partition")
        data_partition_factory = part.DataMemm if memm else part.DataZarr
    seed = config.get("random_seed", 0)
    import random

    import numpy as np
    import torch
    np.random.seed(seed); random.seed(seed); torch.manual_seed(seed)
    segpipe = SegPipeUNet(**config, experiment_name=experiment_name)
    segpipe.load_model_params(checkpoint_path=config["checkpoint_path"])
    if eval_classes == "all":
        eval_classes = parse_classes("all", segpipe.model.n_classes)
    config["eval_classes"] = eval_classes
    print(f'\nLoading {config["data_mode"]} data partition object...')
    t0 = time.time()
    partition = data_partition_factory(**config)
    print(f"Executed time for loading data partition object (min): {round((time.time() - t0) / 60, 2)}")
    run = os.path.normpath(str(config["checkpoint_path"])).split(os.path.sep)[-2]
    config["save_path_metrics"] = os.path.join(str(config["save_path_metrics"]), experiment_name, run)
    config["save_path_plot"] = os.path.join(str(config["save_path_plot"]), experiment_name, run)
    os.makedirs(config["save_path_metrics"], exist_ok=True)
    os.makedirs(config["save_path_plot"], exist_ok=True)
    print("\nMetrics directory:", config["save_path_metrics"])
    print("Plot directory:", config["save_path_plot"], "\n")
    ds, dtf, ltf = factories
    results = {}
    for survey in partition.get_evaluation_surveys():
        readers = partition.get_survey_readers(survey)
        print("Running evaluation for", survey)
        fn = validate_model_survey_memm if memm else validate_model_survey_zarr
        kw = dict(config)
        kw.update(survey=survey, dataset_cls=ds, data_transform_factory=dtf, label_transform_factory=ltf, tiled=tiled)
        results[survey] = fn(readers, segpipe, **kw)
    return results


if __name__ == "__main__":
    main()
