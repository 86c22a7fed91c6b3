"""Range-image segmentation side of the project (reference: semseg/): the SqueezeSegV1 / SqueezeSegV2 trunks with the
reference's module tree and state dict, whose evaluation-mode Fire modules run as one native launch each; the CRF-RNN
refinement layer, the kNN label filter and the training objective -- focal loss under the masked mean, with the step's
predictions and training confusion counts -- on native kernels (semseg.models), the confusion counts / IoU scoring
of an evaluation (semseg.metrics), the frontal-scan datasets (semseg.datasets), the single-GPU training step with
its optimizer tail on native kernels (semseg.trainer, semseg.config; the command line is train_semseg.py) and the
evaluation of a checkpoint (semseg.pretrained, semseg.evaluation; the command line is test_semseg.py), in which V2's
context-aggregation modules run as one native launch each as well."""
