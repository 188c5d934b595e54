from .image_datasets import (PairedImageDataset, PairedImageDatasetConfig, UnpairedImageDataset,  # noqa: F401
                             UnpairedImageDatasetConfig)
from .synthetic import (SyntheticImageDataset, SyntheticImageDatasetConfig,  # noqa: F401
                        SyntheticMaskedImageDataset, SyntheticMaskedImageDatasetConfig, SyntheticSavingImageDataset,
                        SyntheticSavingImageDatasetConfig)
from .multimodal_images import (MultiModalImageDataset, MultiModalImageDatasetConfig,  # noqa: F401
                                MultiModalImageValTestDataset, MultiModalImageValTestDatasetConfig)
from .multimodal_valtest import MultiModalVolumeValTestDataset, MultiModalVolumeValTestDatasetConfig  # noqa: F401
from .multimodal_volumes import MultiModalVolumeDataset, MultiModalVolumeDatasetConfig  # noqa: F401
from .volume_datasets import UnpairedVolumeDataset, UnpairedVolumeDatasetConfig  # noqa: F401
