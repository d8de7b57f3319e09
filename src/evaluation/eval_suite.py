"""Drop-in for the reference's src/evaluation/eval_suite.py: the same public names and the same `evaluate_folder` signature, with
the per-image scores (l1, l2, psnr, ssim as skimage / numpy compute them on 8-bit images) computed by HIP kernels on the device
(diner_amd.evaluate / diner_amd.metrics).  DINER.create_prediction_folder reads the file suffixes through this module, and
create_prediction_folder.py / evaluate_prediction_folder.py / DINER.on_validation_epoch_end call evaluate_folder.

There is no CPU fallback: `device` None means the current HIP device and a CPU device raises RuntimeError.  LPIPS is computed when the
`lpips` package is importable and its VGG weights can be built, or on the device from the file LPIPS_WEIGHTS names (that network's state
dict; `evaluate_folder` keeps the reference's signature, so the path is a module attribute that is passed on as
diner_amd.evaluate.evaluate_folder's `lpips_weights`), and is otherwise left out of the scores with a warning.
`compare_evaluations` (matplotlib comparison plots) is not provided."""
from diner_amd import evaluate as _ev

METRIC_OPT_DICT = dict(l1="-", l2="-", lpips="-", psnr="+", ssim="+")
METRIC_LIMIT_DICT = dict(l1=[0, 0.1], l2=[0, 0.05], lpips=[0., 0.5], psnr=[12, 30], ssim=[.6, 1.])
AVERAGE_SCORE_FILENAME = _ev.AVERAGE_SCORE_FILENAME
REPORT_DETAIL_FILENAME = _ev.REPORT_DETAIL_FILENAME
BARPLOT_FILENAME = "average_scores.png"
EXAMPLE_PLOT_FILENAME = _ev.EXAMPLE_PLOT_FILENAME
N_EXAMPLE_PLOTS = _ev.N_EXAMPLE_PLOTS
PRED_SUFFIX = _ev.PRED_SUFFIX
GT_SUFFIX = _ev.GT_SUFFIX
REF_SUFFIX = _ev.REF_SUFFIX
DEPTH_SUFFIX = _ev.DEPTH_SUFFIX
LPIPS_WEIGHTS = None          # a torch.load-able lpips.LPIPS(net="vgg") state dict: LPIPS then runs on the device (diner_amd.perceptual)


def evaluate_folder(source_dir, outdir, device=None, pred_suffix=PRED_SUFFIX, gt_suffix=GT_SUFFIX,
                    ref_suffix=REF_SUFFIX, depth_suffix=DEPTH_SUFFIX,
                    show_tqdm=False):
    """Scores the -gt / -pred pairs of `source_dir` on the device and writes average_scores.json, detailed_report.json and
    examples.png into `outdir`; returns the averages (see diner_amd.evaluate.evaluate_folder)."""
    return _ev.evaluate_folder(source_dir, outdir, device=device, pred_suffix=pred_suffix, gt_suffix=gt_suffix,
                               ref_suffix=ref_suffix, depth_suffix=depth_suffix, show_tqdm=show_tqdm, lpips_weights=LPIPS_WEIGHTS)


def compare_evaluations(eval_dirs, outdir):
    raise NotImplementedError("compare_evaluations (matplotlib comparison plots of several evaluations) is not provided by this "
                              "project; evaluate_folder's average_scores.json / detailed_report.json hold the numbers to compare")
