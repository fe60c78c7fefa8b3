"""controllable_xgating_amd -- MI355X-native (gfx950) hot path of the gated-fusion caption decoder
(reference: vsislab/Controllable_XGating, caption_src/SAModel.py).  See DESIGN.md.

Environment note (the package never WRITES the environment; it reads two variables, both for tests / tools only: XG_LIBRARY --
another build of the same ABI, _native.py -- and XG_FORCE_DIST -- the collective path on one rank, train.py): a training process uses up to seven HIP
streams (the caller's, the library's two side streams, the optimizer's and the gradient all-reduce's side streams, RCCL's
own) and the ROCm runtime multiplexes streams onto its hardware queues (4 by default); beyond that, independent streams
share a queue and serialise (measured with the data-parallel path on one GPU: 7.44 ms per iteration with 4 queues, 6.18
with 8).  The queue count is the runtime's business: neither this package nor ``bench.py`` changes it."""
from ._native import XgError, lib, LIB_PATH  # noqa: F401,E402
from .model import (SAModel, LanguageModelCriterion, ClassiferCriterion, RewardCriterion, PerVideoRewardCriterion, make_opt)  # noqa: F401,E402
from .control import (pad_templates, caption_with_templates, caption_sampled, caption_beam, first_occurrences,  # noqa: F401,E402
                      beam_captions_with_templates, score_captions_with_templates, template_recovery, allow_masks,
                      beam_captions_following_templates, template_adherence, diverse_beam_captions_with_templates,
                      caption_beam_diverse, caption_truncated_with_templates, length_scale_table, repeated_ngrams,
                      beam_captions_ruled_with_templates)
from .joint import JointTrainer  # noqa: F401,E402

__all__ = ["SAModel", "LanguageModelCriterion", "ClassiferCriterion", "RewardCriterion", "PerVideoRewardCriterion", "make_opt", "XgError", "lib", "pad_templates",
           "caption_with_templates", "caption_sampled", "caption_beam", "first_occurrences", "beam_captions_with_templates",
           "score_captions_with_templates", "template_recovery", "allow_masks", "beam_captions_following_templates",
           "template_adherence", "diverse_beam_captions_with_templates", "caption_beam_diverse",
           "caption_truncated_with_templates", "length_scale_table", "repeated_ngrams", "beam_captions_ruled_with_templates", "JointTrainer"]
