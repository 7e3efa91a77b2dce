from .coco import load_coco_dataset, COCO_CLASS_NAME
from .voc import load_voc_dataset
from .tfcsv import load_tfcsv_dataset
