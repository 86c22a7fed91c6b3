"""Range-image segmentation side of the project (reference: semseg/): the CRF-RNN refinement layer on native kernels."""
