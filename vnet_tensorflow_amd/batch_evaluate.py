"""The reference's utils/batch_evaluate: sweep checkpoints x window strides, evaluate every case, score each result against the ground
truth and write one CSV per combination -- the tool that picks a checkpoint and a stride.

    python -m vnet_tensorflow_amd.batch_evaluate --checkpoint_dir ./tmp/ckpt --data_dir ./data/evaluate --config_json ./config.json ...

What differs from the reference, on purpose:
  * ONE model is built, from config_json; every checkpoint is loaded into it (load_checkpoint(..., with_optimizer=False)) and the stride
    is set on it.  The reference starts `python evaluate.py` with os.system per combination: a new graph every time, every label
    through a file.  Nothing here starts a child process.
  * The score needs no label file: evaluate_single_3D's on_label hook hands over the int32 label while it is still on the device, and
    ops.label_overlap / ops.component_shapes score it there against the case's ground truth (uploaded once per case, remapped through
    SegmentationClasses like data.remap_labels; its component shapes computed once per case).  Only the count table and the component
    rows come to the host.  The rules: vnet_tensorflow_amd/score.py.  Files are written only with write_labels=True, under the name
    evaluate() would use for `evaluated_filename`.
  * All cases run: the reference's exit() after the first case (batch_evaluate.py:300) is a leftover.
  * patch_size / patch_layer reach the model: they replace TrainingSetting.PatchShape by [patch_size, patch_size, patch_layer]; None
    keeps the config's value (the reference's constructor drops both arguments).
  * The flags are parsed from the real command line, not from the string main.py hard-codes; --mode, --tolerance and --gpu are
    added.
  * --mode SURFACE (not in the reference) adds HD, HD95 and ASSD of the foreground surface in physical units, by the rules of score.py;
    on a device model an exact Euclidean distance transform runs there (vnet_tensorflow_amd/surface.py).  A case in which exactly one
    of the two maps has no foreground scores inf, and so does the `average` row.
  * --postprocess PATH (not in the reference) names the YAML of a post-processing pipeline (vnet_tensorflow_amd/postprocess.py) and
    overrides EvaluationSetting.Postprocess: the label is cleaned class by class on the device before on_label hands it over, so the
    scores and the files of write_labels=True are those of the post-processed label.
  * --mirror AXES, --window_weights KIND [KIND ...], --window_sigma S (not in the reference; vnet_tensorflow_amd/window.py): mirrored
    passes and Gaussian window weights of the sliding window.  They override EvaluationSetting.Mirror / WindowWeights / WindowSigma;
    several window weights are a further dimension of the sweep, inside the stride loop.  A CSV keeps the reference's name while the
    weights are uniform and no mirror is set; otherwise the name says so, e.g. `..._window-gaussian_mirror-012.csv`."""
import argparse
import copy
import csv
import json
import os
import re

import numpy as np

from . import data as vdata
from . import score

ITEM_COLUMNS = ["TP", "FP", "FN", "Item Sensitivity", "Item IoU"]
SURFACE_COLUMNS = ["HD", "HD95", "ASSD"]
_CKPT = re.compile(r"^checkpoint-(\d+)(\.index)?$")


def list_checkpoints(folder):
    """[(step, path prefix)] in ascending step order: this project's `checkpoint-<step>` files and the reference's
    `checkpoint-<step>.index` (one entry per step).  `checkpoint-latest`, the pointer file, is never one."""
    found = {}
    for name in os.listdir(folder):
        m = _CKPT.match(name)
        if m and os.path.isfile(os.path.join(folder, name)):
            found[int(m.group(1))] = os.path.join(folder, "checkpoint-%s" % m.group(1))
    return sorted(found.items())


def columns(mode):
    cols = ["Case"]
    if "DICE" in mode:
        cols += ["DICE", "Jaccard"]
    if "ITEM" in mode:
        cols += ITEM_COLUMNS
    if "SURFACE" in mode:
        cols += SURFACE_COLUMNS
    return cols


def write_csv(path, mode, rows):
    """The reference's CSV: `,` delimiter, `|` quote char, QUOTE_MINIMAL; the header, one row per case, and a last row `average` with
    the mean of every numeric column.  Returns the average row."""
    cols = columns(mode)
    avg = {"Case": "average"}
    for c in cols[1:]:
        avg[c] = float(np.mean([r[c] for r in rows])) if rows else 0.0
    if os.path.exists(path):
        os.remove(path)
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, delimiter=",", quotechar="|", quoting=csv.QUOTE_MINIMAL, fieldnames=cols)
        w.writeheader()
        for r in rows:
            w.writerow(r)
        w.writerow(avg)
    return avg


class Batch_Evaluate:
    def __init__(self,
                 config_json="./config.json",
                 model_folder="./tmp/ckpt",
                 output_folder="./tmp",
                 data_folder="./data",
                 ground_truth_filename="label.nii.gz",
                 evaluated_filename="label_vnet.nii.gz",
                 stride_layer_min=32,
                 stride_layer_max=64,
                 stride_inplane_min=32,
                 stride_inplane_max=64,
                 patch_size=64,
                 patch_layer=64,
                 step=2,
                 checkpoint_min=1,
                 checkpoint_max=9999999999999999999999999,
                 batch_size=5,
                 mode=["DICE"],
                 tolerance=3,
                 device=None,
                 write_labels=False,
                 verbose=False,
                 cache_fields=True,
                 postprocess=None,
                 mirror=None,
                 window_weights=None,
                 window_sigma=None):
        self.config_json = config_json               # a path, or the parsed dict
        self.model_folder = model_folder
        self.output_folder = output_folder
        self.data_folder = data_folder

        assert isinstance(ground_truth_filename, str)
        self.ground_truth_filename = ground_truth_filename
        assert isinstance(evaluated_filename, str)
        self.evaluated_filename = evaluated_filename

        for v in (stride_layer_min, stride_layer_max, stride_inplane_min, stride_inplane_max, step, checkpoint_min, checkpoint_max):
            assert isinstance(v, int) and v > 0
        self.stride_layer_min, self.stride_layer_max = stride_layer_min, stride_layer_max
        self.stride_inplane_min, self.stride_inplane_max = stride_inplane_min, stride_inplane_max
        self.step = step
        self.checkpoint_min, self.checkpoint_max = checkpoint_min, checkpoint_max

        assert patch_size is None or (isinstance(patch_size, int) and patch_size > 0)
        assert patch_layer is None or (isinstance(patch_layer, int) and patch_layer > 0)
        self.patch_size, self.patch_layer = patch_size, patch_layer
        self.batch_size = batch_size
        self.mode = list(mode)                       # DICE, ITEM, SURFACE
        assert self.mode and all(m in ("DICE", "ITEM", "SURFACE") for m in self.mode), mode
        self.tolerance = tolerance
        self.device = device
        self.write_labels = bool(write_labels)
        self.verbose = bool(verbose)
        # SURFACE: keep every case's ground-truth surface and its squared distance field (8 bytes per voxel) over the sweep
        self.cache_fields = bool(cache_fields)
        # the YAML of a post-processing pipeline (postprocess.py): overrides EvaluationSetting.Postprocess; None keeps the config's
        assert postprocess is None or isinstance(postprocess, str)
        self.postprocess = postprocess
        # window.py: a flat axis list, the window weights to sweep (one name or several), the Gaussian's sigma; None keeps the config's
        from . import window as vwin
        self.mirror = None if mirror is None else [int(a) for a in mirror]
        if self.mirror is not None:
            vwin.flip_sets(self.mirror)                  # (refuses an axis outside 0 .. 2 and a repeated one, by name)
        if isinstance(window_weights, str):
            window_weights = [window_weights]
        self.window_weights = None if window_weights is None else list(window_weights)
        assert self.window_weights is None or (self.window_weights and len(set(self.window_weights)) == len(self.window_weights) and
                                               all(k in vwin.KINDS for k in self.window_weights)), window_weights
        self.window_sigma = window_sigma

    @property
    def model_folder(self):
        return self._model_folder

    @model_folder.setter
    def model_folder(self, model_folder):
        assert isinstance(model_folder, str)
        self._model_folder = os.path.abspath(model_folder)

    @property
    def output_folder(self):
        return self._output_folder

    @output_folder.setter
    def output_folder(self, output_folder):
        assert isinstance(output_folder, str)
        self._output_folder = os.path.abspath(output_folder)

    @property
    def data_folder(self):
        return self._data_folder

    @data_folder.setter
    def data_folder(self, data_folder):
        assert isinstance(data_folder, str)
        self._data_folder = os.path.abspath(data_folder)

    # ---- the pieces of Execute ----------------------------------------------------------------------------------------------------
    def config(self):
        """The parsed config with the patch arguments applied."""
        if isinstance(self.config_json, dict):
            cfg = copy.deepcopy(self.config_json)
        else:
            with open(self.config_json) as f:
                cfg = json.load(f)
        T = cfg["TrainingSetting"]
        shape = list(T["PatchShape"])
        if self.patch_size is not None:
            shape[0] = shape[1] = int(self.patch_size)
        if self.patch_layer is not None:
            shape[2] = int(self.patch_layer)
        T["PatchShape"] = shape
        if self.postprocess is not None:
            cfg.setdefault("EvaluationSetting", {})["Postprocess"] = self.postprocess
        if self.mirror is not None:
            cfg.setdefault("EvaluationSetting", {})["Mirror"] = list(self.mirror)
        if self.window_sigma is not None:
            cfg.setdefault("EvaluationSetting", {})["WindowSigma"] = self.window_sigma
        return cfg

    def weights(self, model):
        """The window weights of the sweep: the argument's, else the one the config sets on the model."""
        return list(self.window_weights) if self.window_weights is not None else [getattr(model, "evaluate_window_weights", "uniform")]

    @staticmethod
    def csv_name(step, stride_inplane, stride_layer, window_weights="uniform", masks=(0,)):
        """The reference's file name; with other than uniform weights or with mirrored passes, a suffix that says so (the mirror as the
        axes of its masks: `mirror-012` every subset of three axes, `mirror-01` the one joint flip [[0, 1]] or both axes' subsets)."""
        name = "result_checkpoint-%d_stride_inplane-%d_stride_layer-%d" % (step, stride_inplane, stride_layer)
        axes = "".join(str(a) for a in range(3) if any(m >> a & 1 for m in masks))
        if window_weights != "uniform" or axes:
            name += "_window-%s" % window_weights
        if axes:
            name += "_mirror-%s" % axes
        return name + ".csv"

    def build_model(self, cfg):
        """The ONE model of the sweep."""
        from .model import image2label
        m = image2label(None, cfg, device=self.device, verbose=self.verbose)
        m.read_config()
        m.rank, m.local_rank, m.world = 0, 0, 1
        m.build_model_graph()
        return m

    def checkpoints(self):
        return [(s, p) for s, p in list_checkpoints(self._model_folder) if self.checkpoint_min <= s <= self.checkpoint_max]

    def strides(self):
        """The reference's two range(min, max + 1, step) loops, in-plane outside."""
        return [(a, b) for a in range(self.stride_inplane_min, self.stride_inplane_max + 1, self.step)
                for b in range(self.stride_layer_min, self.stride_layer_max + 1, self.step)]

    def cases(self):
        """The case directories that hold the ground truth, in name order."""
        return [c for c in sorted(os.listdir(self._data_folder))
                if os.path.isfile(os.path.join(self._data_folder, c, self.ground_truth_filename))]

    def _case(self, model, name, cache):
        """What a case keeps over the whole sweep: the input image (host), its spacing, the remapped ground truth where the model's
        labels live (uploaded once), for ITEM the ground truth's component shapes (computed once) and, for SURFACE with cache_fields,
        the ground truth's surface and squared distance field (computed once; on the device for a device model)."""
        entry = cache.get(name)
        if entry is None:
            cdir = os.path.join(self._data_folder, name)
            chans = [np.asarray(vdata.load_volume(os.path.join(cdir, f)), dtype=np.float32) for f in model.evaluate_image_filenames]
            gt_path = os.path.join(cdir, self.ground_truth_filename)
            gt = np.ascontiguousarray(vdata.remap_labels(vdata.load_volume(gt_path), model.label_classes))
            if gt.shape != chans[0].shape:
                raise ValueError("%s: ground truth %s, image %s" % (name, gt.shape, chans[0].shape))
            if model.device.type == "cuda":
                import torch
                gt = torch.from_numpy(gt).to(model.device)
            entry = {"dir": cdir, "image": np.stack(chans, axis=-1), "gt": gt,
                     "spacing": vdata.volume_spacing(os.path.join(cdir, model.evaluate_image_filenames[0])),
                     # (the reference sets the ground truth's spacing on the output before it measures)
                     "gt_spacing": vdata.volume_spacing(gt_path),
                     "gt_shapes": score.shapes_of(gt) if "ITEM" in self.mode else None}
            entry["gt_field"] = score.surface_field(gt, entry["gt_spacing"]) if "SURFACE" in self.mode and self.cache_fields else None
            cache[name] = entry
        return entry

    def _score(self, model, entry, label):
        """The hook's side: `label` is the int32 label where the model left it (a device tensor, or an array of a CPU model)."""
        gt = entry["gt"]
        if tuple(label.shape) != tuple(gt.shape) and all(l >= g for l, g in zip(label.shape, gt.shape)):
            # a pipeline without Resample may have padded the case: evaluate() crops the label to the input file's size on the host
            label = label[tuple(slice(0, int(g)) for g in gt.shape)]
        if tuple(label.shape) != tuple(gt.shape):
            raise ValueError("the label is %s, the ground truth %s" % (tuple(label.shape), tuple(gt.shape)))
        if hasattr(label, "contiguous"):
            label = label.contiguous()
        return score.Accuracy(gt, label, spacing=entry["gt_spacing"], tolerence=self.tolerance, mode=self.mode,
                              L=max(2, min(len(model.label_classes), score.MAX_LABELS)), gt_shapes=entry["gt_shapes"],
                              gt_field=entry["gt_field"])

    def Execute(self):
        model = self.build_model(self.config())
        model.evaluate_batch = self.batch_size
        ckpts = self.checkpoints()
        if not ckpts:
            raise FileNotFoundError("no checkpoint-<step> with %d <= step <= %d in %s" % (self.checkpoint_min, self.checkpoint_max,
                                                                                           self._model_folder))
        os.makedirs(self._output_folder, exist_ok=True)
        tf, regrid = model.evaluate_pipeline_transforms()
        cases, cache = self.cases(), {}
        max_dice = max_jaccard = 0
        first = {"ckpt": os.path.basename(ckpts[0][1]), "stride_inplane": self.stride_inplane_min, "stride_layer": self.stride_layer_min}
        from . import window as vwin
        # (set on the model like the stride: a model that read the config holds the same values already)
        if self.mirror is not None:
            model.evaluate_mirror = list(self.mirror)
        if self.window_sigma is not None:
            model.evaluate_window_sigma = self.window_sigma
        mirror = getattr(model, "evaluate_mirror", None) or []
        kinds, masks = self.weights(model), vwin.flip_sets(mirror)
        swept = len(kinds) > 1            # the best-result dictionaries name the window weights and the mirror only when they are swept
        if swept:
            first.update(window_weights=kinds[0], mirror=list(mirror))
        best_dice_result, best_jaccard_result = dict(first), dict(first)
        for step, prefix in ckpts:
            model.load_checkpoint(prefix, with_optimizer=False)
            for (stride_inplane, stride_layer), kind in ((s, k) for s in self.strides() for k in kinds):
                model.evaluate_stride = [stride_inplane, stride_inplane, stride_layer]
                model.evaluate_window_weights = kind
                rows = []
                for name in cases:
                    entry = self._case(model, name, cache)
                    seen = []
                    label, _ = model.evaluate_case(entry["image"], entry["spacing"], tf, regrid,
                                                   on_label=lambda t, e=entry, s=seen: s.append(self._score(model, e, t)))
                    if len(seen) != 1:
                        raise RuntimeError("evaluate_case handed the label over %d times" % len(seen))
                    result = dict(seen[0], Case=name)
                    if "DICE" in self.mode and self.verbose:
                        print("Case: {}, DICE: {}, Jaccard: {}".format(name, result["DICE"], result["Jaccard"]))
                    rows.append(result)
                    if self.write_labels:
                        model.write_label(os.path.join(entry["dir"], self.evaluated_filename), label, entry["spacing"])
                avg = write_csv(os.path.join(self._output_folder, self.csv_name(step, stride_inplane, stride_layer, kind, masks)),
                                self.mode, rows)
                here = {"ckpt": os.path.basename(prefix), "stride_inplane": stride_inplane, "stride_layer": stride_layer}
                if swept:
                    here.update(window_weights=kind, mirror=list(mirror))
                if "DICE" in self.mode:
                    if avg["DICE"] > max_dice:
                        max_dice, best_dice_result = avg["DICE"], here
                    if avg["Jaccard"] > max_jaccard:
                        max_jaccard, best_jaccard_result = avg["Jaccard"], dict(here)
        print("Best DICE result:", best_dice_result)
        print("Best Jaccard result:", best_jaccard_result)
        return best_dice_result, best_jaccard_result


# ---- the reference's utils/batch_evaluate/main.py ----------------------------------------------------------------------------------
def readable_dir(directory):
    """'Type' for argparse - checks that directory exists."""
    if not os.path.isdir(directory):
        raise argparse.ArgumentTypeError("readable_dir:{0} is not a valid path".format(directory))
    if not os.access(directory, os.R_OK):
        raise argparse.ArgumentTypeError("readable_dir:{0} is not a readable dir".format(directory))
    return directory


def get_args(argv=None):
    parser = argparse.ArgumentParser(description="Batch evaluation tool for VNet.")
    parser.add_argument('-v', '--verbose', dest='verbose', help='Show verbose output', action='store_true')
    parser.add_argument('-cd', '--checkpoint_dir', dest='checkpoint_dir', help='Checkpoint folder', type=readable_dir, metavar='DIR',
                        default='./tmp/ckpt', required=True)
    parser.add_argument('-cmin', '--checkpoint_min', dest='checkpoint_min', help='Minimum checkpoint number', type=int, metavar='INT',
                        default=10000)
    parser.add_argument('-cmax', '--checkpoint_max', dest='checkpoint_max', help='Maximum checkpoint number', type=int, metavar='INT',
                        default=999999999999999999999999999999)
    parser.add_argument('-slmin', '--stride_layer_min', dest='stride_layer_min', help='Minimum stride across layers', type=int,
                        metavar='INT', default=32)
    parser.add_argument('-slmax', '--stride_layer_max', dest='stride_layer_max', help='Maximum stride across layers', type=int,
                        metavar='INT', default=64)
    parser.add_argument('-spmin', '--stride_inplane_min', dest='stride_inplane_min', help='Minimum stride across the plane', type=int,
                        metavar='INT', default=32)
    parser.add_argument('-spmax', '--stride_inplane_max', dest='stride_inplane_max', help='Maximum stride across the plane', type=int,
                        metavar='INT', default=64)
    parser.add_argument('-ps', '--patch_size', dest='patch_size', help='Patch size', type=int, metavar='INT', default=64)
    parser.add_argument('-pl', '--patch_layer', dest='patch_layer', help='Patch layer', type=int, metavar='INT', default=64)
    parser.add_argument('-b', '--batch', dest='batch', help='Batch size', type=int, metavar='INT', default=5)
    parser.add_argument('-d', '--data_dir', dest='data_dir', help='Data folder', type=readable_dir, metavar='DIR', default='./data/evaluate')
    parser.add_argument('-gt', '--ground_truth_filename', dest='ground_truth_filename', help='Ground truth filename', type=str,
                        metavar='FILENAME', default="./3DRA_seg.nii.gz")
    parser.add_argument('-e', '--evaluate_filename', dest='evaluate_filename', help='Evaluated filename', type=str, metavar='FILENAME',
                        default="./label_vnet.nii.gz")
    parser.add_argument('-c', '--config_json', dest='config_json', help='Config JSON file', type=str, metavar='FILENAME',
                        default="./config.json")
    parser.add_argument('-o', '--output', dest='output', help='Output directory', type=readable_dir, metavar='DIR', default="./tmp")
    # additions
    parser.add_argument('--mode', dest='mode', help='Scores to compute', nargs='+', choices=["DICE", "ITEM", "SURFACE"],
                        default=["DICE"])
    parser.add_argument('--tolerance', dest='tolerance', help='Centroid distance below which an item is found (ITEM)', type=float,
                        metavar='FLOAT', default=3)
    parser.add_argument('--gpu', dest='gpu', help='Index of the HIP device', type=int, metavar='INT', default=0)
    parser.add_argument('--postprocess', dest='postprocess', help='YAML of a post-processing pipeline (overrides '
                        'EvaluationSetting.Postprocess)', type=str, metavar='PATH', default=None)
    parser.add_argument('--mirror', dest='mirror', help='Axes to mirror: every subset of them is a pass of every batch (overrides '
                        'EvaluationSetting.Mirror)', type=int, nargs='*', choices=[0, 1, 2], metavar='AXIS', default=None)
    parser.add_argument('--window_weights', dest='window_weights', help='Window weights to sweep (overrides '
                        'EvaluationSetting.WindowWeights)', nargs='+', choices=["uniform", "gaussian"], default=None)
    parser.add_argument('--window_sigma', dest='window_sigma', help='Sigma of the gaussian window weights in units of the window size '
                        '(overrides EvaluationSetting.WindowSigma)', type=float, metavar='FLOAT', default=None)
    args = parser.parse_args(argv)
    if args.verbose:
        args_dict = vars(args)
        for key in sorted(args_dict):
            print("{} = {}".format(str(key), str(args_dict[key])))
    return args


def main(args):
    be = Batch_Evaluate(config_json=args.config_json, model_folder=args.checkpoint_dir, output_folder=args.output,
                        data_folder=args.data_dir, ground_truth_filename=args.ground_truth_filename,
                        evaluated_filename=args.evaluate_filename, stride_layer_min=args.stride_layer_min,
                        stride_layer_max=args.stride_layer_max, stride_inplane_min=args.stride_inplane_min,
                        stride_inplane_max=args.stride_inplane_max, patch_size=args.patch_size, patch_layer=args.patch_layer,
                        checkpoint_min=args.checkpoint_min, checkpoint_max=args.checkpoint_max, batch_size=args.batch,
                        mode=args.mode, tolerance=args.tolerance, device="cuda:%d" % args.gpu, verbose=args.verbose,
                        postprocess=args.postprocess, mirror=args.mirror, window_weights=args.window_weights,
                        window_sigma=args.window_sigma)
    return be.Execute()


if __name__ == "__main__":
    main(get_args())
