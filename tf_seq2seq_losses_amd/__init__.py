"""MI355X-native CTC loss (loss, analytic gradient, analytic Hessian) behind the call signature of
alexeytochin/tf_seq2seq_losses.  HIP kernels for gfx950 in csrc/, C ABI in include/ctc_amd.h."""
from .losses import (  # noqa: F401
    classic_ctc_loss,
    simplified_ctc_loss,
    simple_ctc_loss,
    ctc_loss,
    ctc_loss_from_logproba,
    ClassicCtcLossData,
    SimplifiedCtcLossData,
    CtcAlignment,
    classic_ctc_alignment,
    simplified_ctc_alignment,
    ctc_alignment_from_logproba,
    CtcDecoding,
    classic_ctc_greedy_decode,
    simplified_ctc_greedy_decode,
    ctc_greedy_decode_from_logproba,
    CtcBeamDecoding,
    classic_ctc_beam_search,
    simplified_ctc_beam_search,
    ctc_beam_search_from_logproba,
    CtcNbestLoss,
    classic_ctc_nbest_loss,
    simplified_ctc_nbest_loss,
    ctc_nbest_loss_from_logproba,
    CtcNbestAlignment,
    classic_ctc_nbest_alignment,
    simplified_ctc_nbest_alignment,
    ctc_nbest_alignment_from_logproba,
)
from .ops import check_labels  # noqa: F401

__version__ = "0.1.0"
__all__ = ["classic_ctc_loss", "simplified_ctc_loss", "simple_ctc_loss", "ctc_loss", "ctc_loss_from_logproba",
           "ClassicCtcLossData", "SimplifiedCtcLossData", "check_labels",
           "CtcAlignment", "classic_ctc_alignment", "simplified_ctc_alignment", "ctc_alignment_from_logproba",
           "CtcDecoding", "classic_ctc_greedy_decode", "simplified_ctc_greedy_decode", "ctc_greedy_decode_from_logproba",
           "CtcBeamDecoding", "classic_ctc_beam_search", "simplified_ctc_beam_search", "ctc_beam_search_from_logproba",
           "CtcNbestLoss", "classic_ctc_nbest_loss", "simplified_ctc_nbest_loss", "ctc_nbest_loss_from_logproba",
           "CtcNbestAlignment", "classic_ctc_nbest_alignment", "simplified_ctc_nbest_alignment", "ctc_nbest_alignment_from_logproba"]
