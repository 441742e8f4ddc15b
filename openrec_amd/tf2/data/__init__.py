from .dataset import Dataset, InteractionIndex  # noqa: F401
from .temporal import temporal_batches, temporal_evaluation  # noqa: F401
from .autoencoder import autoencoder_batches, autoencoder_evaluation  # noqa: F401
