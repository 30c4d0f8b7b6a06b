"""logit_controls.py: the command-line flags of the controls that act on the logits inside the decode loop -- repetition.py,
biasing.py, truncation.py -- in one place for run.py, summarize.py and transcribe.py."""
import biasing
import repetition
import truncation


def add_arguments(parser) -> None:
    repetition.add_arguments(parser)
    biasing.add_arguments(parser)
    truncation.add_arguments(parser)


def options_from_args(args) -> dict:
    """The DecodingOptions fields of all the flags of `add_arguments`, from the parsed namespace."""
    return dict(**repetition.options_from_args(args.repetition_penalty, args.no_repeat_ngram_size),
                **biasing.options_from_args(args.hotwords, args.hotword_bias, args.hotword_start_bias, args.sequence_bias_file),
                **truncation.options_from_args(args.top_k, args.top_p, args.min_p))
