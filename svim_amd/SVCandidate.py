"""Import-name alias: `from svim_amd.SVCandidate import CandidateDeletion, ...` (src/svim/SVCandidate.py)."""
from .candidates import (Candidate, CandidateDeletion, CandidateInversion, CandidateNovelInsertion, CandidateDuplicationTandem,   # noqa: F401
                         CandidateDuplicationInterspersed, CandidateBreakend)
