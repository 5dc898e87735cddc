"""MI355X build of the prefix-caption model classes of /root/reference/CLIP_prefix_caption/train.py."""
from .decode import KVCache  # noqa: F401
from .model import (CaptionScores, ClipCaptionModel, ClipCaptionPrefix, GPT2LMHeadModel, MLP, MappingType,  # noqa: F401
                    TransformerMapper, evaluate_captions)
from .metrics import corpus_bleu_mean, sentence_bleu  # noqa: F401
from .generate import (caption_attention_map, generate2, generate2_batch, generate_beam, generate_beam_batch,  # noqa: F401
                       generate_sample, generate_sample_batch)
from .pipeline import Captioner, PendingCaptions, build_attribute_table  # noqa: F401
from .weights import (CaptionGeometry, GPT2_MODELS, init_caption_state_dict, init_transformer_mapper_state_dict,  # noqa: F401
                      synthetic_caption_batch)
