"""MI355X-native sentence-boundary tagger: drop-in for the tagger hot path of Ighina/MultimodalTopicSegmentation.

Importing this package loads libmts_hip.so (hand-written HIP kernels for gfx950) and fails loudly if it is missing;
there is no CPU or PyTorch fallback for the tagger arithmetic.
"""
from . import _lib  # noqa: F401  (raises ImportError when the HIP library is not built)
from .encoder_dataset import AudioPortionDataset, AudioPortionDatasetInference  # noqa: F401
from .datasets import load_dataset_for_inference, load_dataset_from_precomputed, second_input_of  # noqa: F401
from .lightning_model import TextSegmenter  # noqa: F401
from .prefetch import DevicePrefetcher  # noqa: F401
from .resident import AugmentedCorpus, DocumentShardSampler, MaskedCorpus, ResidentCorpus  # noqa: F401
from .rnn_taggers import BiLSTM, BiLSTMLateFusion, BiRnnCrf, SheikhBiLSTM, SwitchBiLSTM  # noqa: F401
from .t5_taggers import RecurrentLongT5  # noqa: F401
from .crf_taggers import TransformerCRF  # noqa: F401
from .taggers import RestrictedTransformerEncoderLayer, Transformer_segmenter  # noqa: F401
from .threshold_search import DEFAULT_THRESHOLDS, ThresholdSweep  # noqa: F401
from .fit import fit  # noqa: F401
from .evaluate import bootstrap_ci, cross_validate, evaluate, paired_bootstrap  # noqa: F401
from .predict import Prediction, predict, segment_audio  # noqa: F401
from .pca import PcaReducer, pca_from_moments, project_folds  # noqa: F401
from .frames import POOL_MODES, ResidentFrames, load_frames  # noqa: F401
from .audio import ResidentAudio, beta_probs, load_wav, pyin_tables, uniform_spans  # noqa: F401
from .wav2vec2 import Wav2Vec2Weights  # noqa: F401
from .text import ResidentText, TextEncoderWeights, tokenize_documents  # noqa: F401

__all__ = ['TextSegmenter', 'Transformer_segmenter', 'BiLSTM', 'BiLSTMLateFusion', 'BiRnnCrf', 'TransformerCRF', 'RecurrentLongT5', 'SheikhBiLSTM', 'SwitchBiLSTM', 'AudioPortionDataset',
           'AudioPortionDatasetInference', 'RestrictedTransformerEncoderLayer', 'DevicePrefetcher', 'ThresholdSweep', 'DEFAULT_THRESHOLDS', 'ResidentCorpus',
           'DocumentShardSampler', 'AugmentedCorpus', 'MaskedCorpus', 'fit', 'evaluate', 'bootstrap_ci', 'paired_bootstrap', 'cross_validate', 'Prediction', 'predict', 'segment_audio', 'PcaReducer',
           'pca_from_moments', 'project_folds', 'POOL_MODES', 'ResidentFrames', 'load_frames', 'ResidentAudio', 'load_wav', 'uniform_spans', 'pyin_tables', 'beta_probs', 'Wav2Vec2Weights',
           'ResidentText', 'TextEncoderWeights', 'tokenize_documents']
