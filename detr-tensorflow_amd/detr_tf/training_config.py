"""Training configuration of the drop-in API.

Same attribute names, defaults and command-line flags as the reference's
detr_tf/training_config.py (:6-38 flags, :41-77 attributes, :79-103 helpers, :106-112
DataConfig), but plain Python: the learning rates are `LRVar` cells (the reference uses
tf.Variable so that scripts can `.assign()` new values between epochs, finetune_voc.py:76-96).
"""
import argparse
import os


class LRVar:
    """Mutable scalar read at every optimiser step (stand-in for tf.Variable(lr))."""

    def __init__(self, value):
        self.value = float(value)

    def assign(self, value):
        self.value = float(value)
        return self

    def numpy(self):
        return self.value

    def __float__(self):
        return self.value

    def __repr__(self):
        return f"LRVar({self.value})"


# flag, type, default, is_switch   (the reference types the three lr flags as bool -- a defect;
# they are floats here)
_FLAGS = (
    ("data_dir", str, None, False), ("img_dir", str, None, False), ("ann_file", str, None, False),
    ("ann_dir", str, None, False), ("background_class", int, 0, False),
    ("train_backbone", None, False, True), ("train_transformers", None, False, True),
    ("train_nlayers", None, False, True), ("finetuning", None, False, True),
    ("batch_size", int, 1, False), ("gradient_norm_clipping", float, 0.1, False),
    ("target_batch", int, None, False),
    ("backbone_lr", float, 1e-5, False), ("transformers_lr", float, 1e-4, False), ("nlayers_lr", float, 1e-4, False),
    ("log", None, False, True),
    # not in the reference: AdamW decay, one model-wide gradient norm, Adam's epsilon (optimizers.py)
    ("weight_decay", float, 0.0, False), ("global_clipnorm", float, None, False), ("adam_epsilon", float, 1e-7, False),
    # not in the reference (it compiles these in): the set criterion, named after the original DETR's flags (loss/loss.py criterion_of)
    ("set_cost_class", float, 1.0, False), ("set_cost_bbox", float, 5.0, False), ("set_cost_giou", float, 2.0, False),
    ("class_loss_coef", float, 1.0, False), ("bbox_loss_coef", float, 5.0, False), ("giou_loss_coef", float, 2.0, False),
    ("eos_coef", float, 0.1, False), ("num_boxes_min_one", None, False, True),
    # not in the reference: the class term of the criterion, "softmax" (the reference's) or "focal" (sigmoid focal loss)
    ("class_criterion", str, "softmax", False), ("focal_alpha", float, 0.25, False), ("focal_gamma", float, 2.0, False),
    # not in the reference: an exponential moving average of the weights kept on the device (optimizers.WeightEMA)
    ("ema_decay", float, None, False), ("ema_warmup", None, False, True),
)


def training_config_parser():
    parser = argparse.ArgumentParser(description="DETR training options (override TrainingConfig attributes)")
    for name, typ, default, switch in _FLAGS:
        if switch:
            parser.add_argument(f"--{name}", action="store_true", default=default, required=False)
        else:
            parser.add_argument(f"--{name}", type=typ, default=default, required=False)
    return parser


_DEFAULTS = dict(
    data_dir=None, img_dir=None, ann_dir=None, ann_file=None,
    background_class=0, image_size=(376, 672),
    train_backbone=False, train_transformers=False, train_nlayers=False,
    finetuning=False, batch_size=1, gradient_norm_clipping=0.1, target_batch=1,
    global_step=0, log=False, normalized_method="torch_resnet",
    # Optimiser extensions, all read at EVERY step.  weight_decay: decoupled (AdamW) decay of every trained tensor.
    # global_clipnorm: clip by ONE L2 norm over all tensors of the trained groups; when it is not None it REPLACES the
    # per-tensor gradient_norm_clipping ("global wins": Keras refuses both, but gradient_norm_clipping defaults to 0.1 here).
    weight_decay=0.0, global_clipnorm=None, adam_epsilon=1e-7,
    # The set criterion, read at EVERY step (loss/loss.py criterion_of): the matcher's cost = set_cost_bbox * L1 - set_cost_class * prob
    # - set_cost_giou * GIoU, the total = class_loss_coef * label_cost + giou_loss_coef * giou_loss + bbox_loss_coef * l1_loss per
    # level, eos_coef = the cross-entropy weight of an unmatched query, num_boxes_min_one = divide the box sums by max(matched, 1)
    # (a batch without targets then has a finite total).  class_weights (no flag): a sequence of nb_class weights of the MATCHED
    # targets' classes, rounded to multiples of 1/64 in [0, 16].  At these defaults the loss runs the reference's compiled-in criterion.
    set_cost_class=1.0, set_cost_bbox=5.0, set_cost_giou=2.0, class_loss_coef=1.0, bbox_loss_coef=5.0, giou_loss_coef=2.0,
    eos_coef=0.1, num_boxes_min_one=False, class_weights=None,
    # class_criterion = "focal" swaps the class term for the sigmoid focal loss of Deformable DETR and its successors: every one of
    # the nb_class logits a binary problem (matched queries one-hot on their class, unmatched ones all zero), focal_alpha in (0, 1)
    # the weight of the positives, focal_gamma in [0, 8] the focusing exponent; the level's sum is divided by max(matched, 1),
    # eos_coef is not read and class_weights must stay None.  The matcher's class cost becomes the focal cost (the published
    # set_cost_class for it is 2; the default stays 1) and detections are scored by the sigmoid of the best non-background logit
    # (inference.py scoring="sigmoid", what Detector and eval_model choose from this attribute).  Call model.set_class_prior() on a
    # fresh head.  The defaults 0.25 / 2 are the published ones, untuned here.
    class_criterion="softmax", focal_alpha=0.25, focal_gamma=2.0,
    # Weight average (tf.train.ExponentialMovingAverage), read at EVERY apply step.  ema_decay = d, 0 <= d < 1: after the update of
    # the trained groups, shadow -= (1 - d) * (shadow - weights) on the device; None = no average (nothing allocated, nothing
    # launched; setting it back to None pauses the updates and keeps the shadow).  ema_warmup: this step's decay is
    # min(d, (1 + n) / (10 + n)), n = updates done so far (TensorFlow's num_updates rule).
    ema_decay=None, ema_warmup=False,
)


class TrainingConfig:
    def __init__(self):
        for k, v in _DEFAULTS.items():
            setattr(self, k, v)
        self.data = DataConfig()
        self.backbone_lr = LRVar(1e-5)
        self.transformers_lr = LRVar(1e-4)
        self.nlayers_lr = LRVar(1e-4)
        self.nlayers = []

    def add_nlayers(self, layers):
        """Register the names of the freshly added head layers (they form the 'nlayers' group)."""
        self.nlayers = [layer.name for layer in layers]

    def update_from_args(self, args):
        for key, value in vars(args).items():
            cur = getattr(self, key, None)
            if isinstance(cur, LRVar):
                cur.assign(value)
            else:
                setattr(self, key, value)
        self.data = DataConfig(self.data_dir, self.img_dir, self.ann_file, self.ann_dir)


class DataConfig:
    """Joins the dataset paths (reference :106-112)."""

    def __init__(self, data_dir=None, img_dir=None, ann_file=None, ann_dir=None):
        def join(leaf):
            return os.path.join(data_dir, leaf) if (data_dir is not None and leaf is not None) else None
        self.data_dir = data_dir
        self.img_dir = join(img_dir)
        self.ann_file = join(ann_file)
        self.ann_dir = join(ann_dir)
