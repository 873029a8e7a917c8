"""A deterministic stand-in for CLIPTokenizer in the long-prompt tests and in tests/golden/make_golden_long_prompt.py (the real
tokenizer's vocabulary cannot be fetched offline): a prompt is a run of decimal numbers, every number one token.  It honours the two
call forms the product uses -- the reference's long-prompt form (truncation=False, add_special_tokens=False -> plain lists) and the
padded / truncated [B, max_length] form."""
import numpy as np


class StubTokenizer:
    def __init__(self, vocab: int):
        self.vocab = vocab
        self.bos_token_id = vocab - 2
        self.eos_token_id = vocab - 1
        self.pad_token_id = vocab - 1
        self.model_max_length = 77

    def raw(self, text):
        return [int(w) % (self.vocab - 2) for w in text.split()]

    def __call__(self, texts, truncation=True, add_special_tokens=True, padding=None, max_length=None, return_tensors=None):
        texts = [texts] if isinstance(texts, str) else list(texts)
        if not add_special_tokens:
            assert truncation is False and padding is None
            return {"input_ids": [self.raw(t) for t in texts]}
        L = max_length or self.model_max_length
        ids = np.full((len(texts), L), self.pad_token_id, np.int64)
        for b, t in enumerate(texts):
            x = ([self.bos_token_id] + self.raw(t))[:L - 1] + [self.eos_token_id]
            ids[b, :len(x)] = x
        return {"input_ids": ids}


def prompt_of(n_tokens: int, seed: int, vocab: int) -> str:
    """a prompt of n_tokens seeded tokens"""
    g = np.random.default_rng(seed)
    return " ".join(str(int(t)) for t in g.integers(0, vocab - 2, n_tokens))


TOKEN_COUNTS = (0, 74, 75, 76, 150, 226, 300)   # empty; one short of / exactly / one past a window; two windows; one past three; dropped tail
