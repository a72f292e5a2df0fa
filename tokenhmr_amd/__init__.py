"""tokenhmr_amd: TokenHMR on HIP.  The submodules are imported where they are used; the PNG drop-ins are reachable from here by name."""
_PNG_EXPORTS = ("PNGEncoder", "imwrite", "imwrite_batch", "PNGDecoder", "imread")
__all__ = list(_PNG_EXPORTS)


def __getattr__(name):
    if name in _PNG_EXPORTS:         # resolved on first use: importing the package stays free of torch
        from . import png
        return getattr(png, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
