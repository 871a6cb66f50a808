"""Node layouts of the reference's ``pathpyG.visualisations`` (:mod:`.layout`).  Rendering — ``plot``, the backends and their templates — is
not part of this package.  ``visualisations.layout`` is the module; the function of the same name inside it is ``pp.layout``."""
from . import layout  # noqa: F401
from .layout import Layout  # noqa: F401
