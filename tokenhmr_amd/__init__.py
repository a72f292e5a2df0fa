"""tokenhmr_amd: TokenHMR on HIP.  The submodules are imported where they are used; the PNG drop-ins and the tokenizer's reconstruction loss
are reachable from here by name."""
_PNG_EXPORTS = ("PNGEncoder", "imwrite", "imwrite_batch", "PNGDecoder", "imread")
_LOSS_EXPORTS = ("PoseReConsLoss",)
__all__ = list(_PNG_EXPORTS + _LOSS_EXPORTS)


def __getattr__(name):
    if name in _PNG_EXPORTS:         # resolved on first use: importing the package stays free of torch
        from . import png
        return getattr(png, name)
    if name in _LOSS_EXPORTS:
        from . import tokenizer_loss
        return getattr(tokenizer_loss, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
