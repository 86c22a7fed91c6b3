"""Range-image segmentation side of the project (reference: semseg/): the CRF-RNN refinement layer and the kNN label
filter on native kernels (semseg.models), and the confusion counts / IoU scoring of an evaluation (semseg.metrics)."""
