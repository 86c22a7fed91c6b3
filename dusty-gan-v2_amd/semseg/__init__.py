"""Range-image segmentation side of the project (reference: semseg/): the CRF-RNN refinement layer, the kNN label
filter and the training objective -- focal loss under the masked mean, with the step's predictions and training
confusion counts -- on native kernels (semseg.models), and the confusion counts / IoU scoring of an evaluation
(semseg.metrics)."""
